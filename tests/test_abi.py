"""The C-ABI library loads and exports every symbol include/bppo.h declares
(no compute calls: this runs without a GPU)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def so():
    p = os.path.join(ROOT, "burn-ppo_amd", "bppo", "libbppo.so")
    if not os.path.exists(p):
        subprocess.run(["make", "-j8", "-C", os.path.join(ROOT, "burn-ppo_amd")], check=True)
    return p


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "bppo.h")).read()
    return sorted(set(re.findall(r"\b(bppo_[a-z_0-9]+)\s*\(", txt)))


def test_header_declares_expected_surface():
    syms = header_symbols()
    import bppo._lib as L
    assert sorted(L.EXPORTS) == syms


def test_library_exports_every_header_symbol(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (bppo_[a-z_0-9]+)$", out, re.M))
    missing = [s for s in header_symbols() if s not in exported]
    assert not missing, missing


def test_library_loads_and_reports_version(so):
    import bppo._lib as L
    lib = L.lib()
    assert lib.bppo_version().decode().startswith("bppo-mi355x")


def test_offload_arch_is_gfx950(so):
    # the embedded clang offload bundle names its targets (no extraction to disk)
    data = open(so, "rb").read()
    assert b"hipv4-amdgcn-amd-amdhsa--gfx950" in data


def test_host_libm_path_without_gpu():
    import numpy as np
    import bppo._lib as L
    x = np.linspace(1e-6, 1.0, 1000, dtype=np.float32)
    y = np.zeros_like(x)
    assert L.lib().bppo_debug_libm(0, 0, x.ctypes.data, y.ctypes.data, x.size) == 0
    assert np.allclose(y, np.log(x), rtol=1e-6, atol=1e-7)


def test_device_memory_counters_start_at_zero(so):
    """bppo_debug_device_memory makes no HIP call; a fresh process that has created nothing
    holds no allocation and no byte"""
    code = ("import sys, ctypes as C; sys.path.insert(0, sys.argv[1]); import bppo._lib as L; "
            "a, b = C.c_int64(-1), C.c_int64(-1); "
            "print(L.lib().bppo_debug_device_memory(C.byref(a), C.byref(b)), a.value, b.value)")
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "burn-ppo_amd")], capture_output=True,
                         text=True, check=True).stdout
    assert out.split() == ["0", "0", "0"], out
    import bppo._lib as L
    assert L.lib().bppo_debug_device_memory(None, None) == L.ERR_ARG


# ------------------------------------------------------------ struct layouts ---
_C_TYPES = {"int32_t": ("i32", C.c_int32), "float": ("f32", C.c_float), "double": ("f64", C.c_double),
            "uint64_t": ("u64", C.c_uint64)}
_CONSTS = {"BPPO_MAX_PLAYERS": 6}


def _header_struct(name):
    """[(field, type, array_len or 0)] of `typedef struct { ... } name;` in include/bppo.h"""
    txt = open(os.path.join(ROOT, "include", "bppo.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, txt).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, rest = decl.split(None, 1)
        for f in rest.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[(\w+)\])?\s*", f)
            n = 0 if m.group(2) is None else int(_CONSTS.get(m.group(2), m.group(2)))
            out.append((m.group(1), _C_TYPES[ty][0], n))
    return out


def _ctypes_struct(cls):
    inv = {v[1]: v[0] for v in _C_TYPES.values()}
    out = []
    for f, t in cls._fields_:
        if hasattr(t, "_length_"):
            out.append((f, inv[t._type_], t._length_))
        else:
            out.append((f, inv[t], 0))
    return out


def _rust_struct(name):
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    i = txt.index("pub struct %s {" % name) + len("pub struct %s {" % name)
    body = re.sub(r"//[^\n]*", "", txt[i:txt.index("}", i)])
    out = []
    for m in re.finditer(r"pub (\w+):\s*(\[\s*(\w+)\s*;\s*(\d+)\s*\]|\w+)", body):
        if m.group(3):
            out.append((m.group(1), m.group(3), int(m.group(4))))
        else:
            out.append((m.group(1), m.group(2), 0))
    return out


@pytest.mark.parametrize("c_name,rust_name,attr", [
    ("bppo_config", "BppoConfig", "Config"), ("bppo_update_metrics", "BppoUpdateMetrics", "UpdateMetrics"),
    ("bppo_episode", "BppoEpisode", "Episode"), ("bppo_rollout_info", "BppoRolloutInfo", "RolloutInfo")])
def test_struct_layouts_match_header(so, c_name, rust_name, attr):
    """include/bppo.h, the ctypes binding (bppo/_lib.py) and the Rust binding in
    INTEGRATION.md list the same fields, in the same order, with the same types; and the
    library's sizeof exports equal the ctypes sizes."""
    import bppo._lib as L
    hdr = _header_struct(c_name)
    assert _ctypes_struct(getattr(L, attr)) == hdr
    assert _rust_struct(rust_name) == hdr
    size_fn = {"bppo_config": "bppo_config_size", "bppo_update_metrics": "bppo_update_metrics_size",
               "bppo_episode": "bppo_episode_size", "bppo_rollout_info": "bppo_rollout_info_size"}[c_name]
    assert getattr(L.lib(), size_fn)() == C.sizeof(getattr(L, attr))


@pytest.mark.parametrize("preset,over", [
    ("cartpole", dict(split_networks=True, num_hidden=8)),                         # 2 * 8 + 2 = 18 layers
    ("connect_four", dict(hidden_size=32, num_hidden=15)),                         # 17
    ("liars_dice_ctde", dict(num_hidden=8, critic_num_hidden=7)),                  # 17
    ("connect_four", dict(network_type="cnn", split_networks=True, num_conv_layers=4,
                          conv_channels=[4], cnn_num_fc_layers=4))])               # 2 * 8 + 2 = 18
def test_create_rejects_nets_over_16_layers_before_any_hip_call(so, preset, over):
    """NetLayout holds 16 layers; deeper nets (any net type) are refused with
    BPPO_ERR_UNSUPPORTED by bppo_create's configuration check, which runs before the
    first HIP call (so this runs without a GPU)."""
    import bppo
    import bppo._lib as L
    from bppo.host import to_struct
    cfg = bppo.make_config(preset, num_envs=8, num_steps=4, **over)
    s = to_struct(cfg)
    h = C.c_void_p()
    st = L.lib().bppo_create(C.byref(s), 0, None, C.byref(h))
    try:
        assert st == L.ERR_UNSUPPORTED, (st, L.lib().bppo_last_error(h))
        assert b"16 layers" in L.lib().bppo_last_error(h)
    finally:
        L.lib().bppo_destroy(h)


def test_debug_return_norm_rejects_bad_arguments_before_any_hip_call(so):
    """bppo_debug_return_norm checks P (1..BPPO_MAX_PLAYERS), its sizes and its required
    pointers before the first HIP call, so BPPO_ERR_ARG comes back without a GPU."""
    import numpy as np
    import bppo._lib as L
    T, N = 3, 4
    f = np.zeros(T * N, np.float32); pl = np.zeros(T * N, np.int32)
    R = np.zeros(N * 6); st = np.zeros(3); allr = np.zeros(T * N * 6, np.float32)

    def call(T=T, N=N, P=2, raw=f, done=f, players=pl, valid=None, R=R, st=st, rew=f, allr=allr):
        p = [None if a is None else a.ctypes.data for a in (raw, done, players, valid, R, st, rew, allr)]
        return L.lib().bppo_debug_return_norm(T, N, P, 0.99, 10.0, *p)

    for bad in (dict(P=0), dict(P=-1), dict(P=7), dict(T=0), dict(N=0), dict(raw=None), dict(done=None),
                dict(R=None), dict(st=None), dict(rew=None),
                dict(players=None, P=2, allr=None),               # the single-player kernel is P = 1
                dict(players=None, P=1, allr=None, valid=f),      # ... without valid
                dict(players=None, P=1)):                         # ... or all_rewards
        assert call(**bad) == L.ERR_ARG, bad


def test_debug_update_kernel_hooks_reject_bad_arguments_before_any_hip_call(so):
    """bppo_debug_adv_stats, bppo_debug_slab_reduce and bppo_debug_adam check their sizes, their
    required pointers and the reduction scratch's capacity before the first HIP call, so
    BPPO_ERR_ARG / BPPO_ERR_UNSUPPORTED come back without a GPU."""
    import numpy as np
    import bppo._lib as L
    lib = L.lib()
    ptr = lambda a: None if a is None else a.ctypes.data

    B, M = 8, 2
    adv = np.zeros(B, np.float32); perm = np.arange(B, dtype=np.uint32); stats = np.zeros((M, 4), np.float32)
    path = C.c_int32(-1)

    def adv_call(B=B, M=M, adv=adv, perm=perm, inv=perm, stats=stats, path=C.byref(path)):
        return lib.bppo_debug_adv_stats(B, M, ptr(adv), ptr(perm), ptr(inv), ptr(stats), path)

    out_of_range = perm.copy(); out_of_range[3] = B
    for bad in (dict(B=0), dict(M=0), dict(M=-1), dict(adv=None), dict(perm=None), dict(stats=None), dict(path=None),
                dict(perm=out_of_range), dict(inv=out_of_range)):
        assert adv_call(**bad) == L.ERR_ARG, bad
    # one row per block over the permutation (B < M): 600 blocks of 8 partials exceed the scratch
    big = np.arange(600, dtype=np.uint32)
    assert adv_call(B=600, M=601, adv=np.zeros(600, np.float32), perm=big, inv=None,
                    stats=np.zeros((601, 4), np.float32)) == L.ERR_UNSUPPORTED

    slab = np.zeros((2, 16), np.float32); grad = np.zeros(16 + 64, np.float32); vm = np.zeros(1, np.float32)

    def slab_call(rows=2, width=16, slab=slab, grad=grad, vm=vm):
        return lib.bppo_debug_slab_reduce(rows, width, ptr(slab), ptr(grad), ptr(vm))

    for bad in (dict(rows=0), dict(rows=-1), dict(width=10), dict(width=0), dict(slab=None), dict(grad=None),
                dict(vm=None)):
        assert slab_call(**bad) == L.ERR_ARG, bad

    lens = np.array([4, 2], np.int32); f = np.zeros(6, np.float32)
    tail = np.zeros(15, np.float32); st4 = np.zeros(4, np.float32); row = np.zeros(18, np.float32)

    def adam_call(nt=2, lens=lens, step=1, world=1, fused=0, grad=f, params=f, m1=f, m2=f, tail=tail, st4=st4, nm=14,
                  row=row):
        return lib.bppo_debug_adam(nt, ptr(lens), step, world, 1e-3, 0.5, 1e-5, fused, ptr(grad), ptr(params), ptr(m1),
                                   ptr(m2), ptr(tail), ptr(st4), nm, ptr(row))

    for bad in (dict(nt=0), dict(nt=-1), dict(nt=33), dict(lens=None), dict(lens=np.array([4, 0], np.int32)),
                dict(step=0), dict(world=0), dict(fused=2), dict(grad=None), dict(params=None), dict(m1=None),
                dict(m2=None), dict(tail=None), dict(st4=None), dict(row=None), dict(nm=-1), dict(nm=15),
                dict(fused=1, lens=np.array([4097, 2], np.int32))):      # fused: every tensor within one chunk
        assert adam_call(**bad) == L.ERR_ARG, bad
    # 32 tensors of 131 chunks each: 4192 block partials, the scratch holds 4160 -- refused before
    # any buffer is read (the arrays above are far smaller than the table)
    assert adam_call(nt=32, lens=np.full(32, 131 * 4096, np.int32)) == L.ERR_UNSUPPORTED


def test_null_context_is_an_argument_error(so):
    """every setter checks its context before touching it (bppo_optimizer_set
    dereferenced a NULL ctx); no HIP call is made, so this runs without a GPU."""
    import bppo._lib as L
    lib = L.lib()
    buf = (C.c_float * 4)()
    steps = (C.c_int32 * 4)()
    assert lib.bppo_optimizer_set(None, buf, buf, steps, 4) == L.ERR_ARG
    assert lib.bppo_optimizer_get(None, buf, buf, steps, 4) == L.ERR_ARG
    assert lib.bppo_params_set(None, buf, 4) == L.ERR_ARG
    assert lib.bppo_rng_set(None, 0) == L.ERR_ARG
    assert lib.bppo_set_explained_variance_mode(None, 1) == L.ERR_ARG
    assert lib.bppo_set_minibatch_kernel(None, 2) == L.ERR_ARG
