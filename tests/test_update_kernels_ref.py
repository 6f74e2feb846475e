"""What tests/test_gpu_update_kernels.py relies on, settled without a GPU: every case of its
tables stays inside the fragile-output cap under the seed the table names (update_kernels_ref.py
states the rule), the Adam cases' f32 norms are not fragile at all, the numpy restatement of the
clip + Adam step equals the oracle's or_adam_step bit for bit, and the constants the tables are
built around are the kernels' own."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_ffi as O
import update_kernels_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_kernels_own():
    src = open(os.path.join(ROOT, "burn-ppo_amd", "csrc", "k_update.hip")).read()
    hdr = open(os.path.join(ROOT, "burn-ppo_amd", "csrc", "bppo_internal.h")).read()
    slots = re.search(r"enum \{ (M_PL = 0[^}]*) \};", src).group(1).replace(" = 0", "").split(", ")
    assert slots.index("NUM_M") == R.NUM_M and slots.index("M_VEMAX") == R.M_VEMAX
    for name, text in (("ADAM_CHUNK", src), ("SLAB_GROUPS", src), ("SLAB_GUARD", src), ("ADV_STREAM_BLOCKS", hdr),
                       ("ADV_STREAM_MAXM", hdr), ("GRAD_METRIC_SLOTS", hdr), ("GRAD_VEMAX", hdr)):
        assert int(re.search(r"\b%s = (\d+)" % name, text).group(1)) == getattr(R, name), name
    assert "RED_SCRATCH_DOUBLES = 4 * 1024 + 64;" in hdr and "GRAD_VEMAX_LOCAL = GRAD_METRIC_SLOTS" in hdr


def test_adv_case_table_reaches_every_branch():
    paths = {R.adv_plan(B, M, True)[0] for B, M in R.ADV_CASES}
    assert paths == {0, 4, 8, 16}
    for w in (4, 8, 16):
        splits = {B % M == 0 for B, M in R.ADV_CASES if R.adv_plan(B, M, True)[0] == w}
        assert splits == {True, False}, w
    for B in {B for B, _ in R.ADV_CASES}:
        assert any(b == B and B % M for b, M in R.ADV_CASES), B           # every B meets a ragged M
    assert any(B < M for B, M in R.ADV_CASES)                             # base == 0
    for have_inv in (True, False):                                        # more than one load round
        _, Cc, _ = R.adv_plan(R.BIG, 3, have_inv)
        assert Cc > 4096
    capped = [(B, M) for B, M in R.ADV_CASES if B // M and (B + 511) // 512 > B // M]
    assert (51282, 518) in capped and (65537, 512) in capped

    def mb_of(i, B, M):
        base, rem = B // M, B % M
        return i // (base + 1) if i < rem * (base + 1) else rem + (i - rem * (base + 1)) // base

    B, M = 51282, 518                       # without the cap a block would meet three minibatches
    C0 = (B + 511) // 512
    assert any(mb_of(min(b + C0, B) - 1, B, M) - mb_of(b, B, M) >= 2 for b in range(0, B, C0))
    for B, M in R.ADV_CASES:
        assert R.adv_plan(B, M, False)[2] * 8 <= R.RED_SCRATCH_DOUBLES


@pytest.mark.parametrize("B,M", R.ADV_CASES)
def test_adv_cases_stay_inside_the_fragile_cap(B, M):
    for kind in R.adv_kinds(B):
        n = R.adv_fragile_count(R.adv_reference(B, M, kind))
        assert n <= R.fragile_cap(M), (kind, n)


def test_adv_empty_minibatch_is_nan_in_the_oracle_too():
    """or_normalize_advantages on n = 0 rows: mean 0 / 0 and the variance are NaN, min / max
    stay +inf / -inf; on n = 1 the mean is the row and the std NaN"""
    st = [C.c_float() for _ in range(4)]
    O.lib().or_normalize_advantages(np.zeros(1, np.float32), 0, np.zeros(1, np.float32), *[C.byref(x) for x in st])
    assert np.isnan(st[0].value) and np.isnan(st[1].value) and st[2].value == np.inf and st[3].value == -np.inf
    O.lib().or_normalize_advantages(np.full(1, 3.5, np.float32), 1, np.zeros(1, np.float32), *[C.byref(x) for x in st])
    assert st[0].value == 3.5 and np.isnan(st[1].value) and st[2].value == st[3].value == 3.5


@pytest.mark.parametrize("B,M,kind", [(1000, 3, "n01"), (1000, 12, "mean1000"), (513, 8, "planted"), (4099, 5, "mean10")])
def test_adv_reference_is_the_oracles(B, M, kind):
    """the exact two-pass reference against or_normalize_advantages (sequential f64 sums): min and
    max equal, mean equal unless fragile, std within one ulp"""
    adv, perm, _ = R.adv_inputs(B, M, kind)
    for (s, e), r in zip(R.mb_bounds(B, M), R.adv_reference(B, M, kind)):
        st = [C.c_float() for _ in range(4)]
        O.lib().or_normalize_advantages(np.ascontiguousarray(adv[perm[s:e]]), e - s, np.zeros(e - s, np.float32),
                                        *[C.byref(x) for x in st])
        assert st[2].value == r["min"] and st[3].value == r["max"]
        assert R.ulps_apart(st[0].value, r["mean"]) <= (1 if R.fragile(r["mean"], r["mabs"], r["n"]) else 0)
        assert R.ulps_apart(st[1].value, r["std"]) <= 1


@pytest.mark.parametrize("rows,width", R.SLAB_CASES)
def test_slab_cases_stay_inside_the_fragile_cap(rows, width):
    n = R.slab_fragile_count(rows, width)
    assert n <= R.fragile_cap(width), n


@pytest.mark.parametrize("name", list(R.ADAM_TABLES))
def test_adam_case_norms_are_not_fragile(name):
    lens = R.ADAM_TABLES[name]
    seen = set()
    for c in R.adam_chain(name):
        for t, ss in enumerate(R.adam_norms(lens, c["grad"], c["world"])):
            assert not R.norm_fragile(ss, lens[t]), (c["step"], c["kind"], t)
        seen |= {(bool(ss == 0), cl) for ss, cl in zip(R.adam_norms(lens, c["grad"], c["world"]), c["clipped"])}
    assert seen == {(True, False), (False, True), (False, False)}       # zero, far above, far below


def test_adam_threshold_cases():
    for k, g, want in R.threshold_cases():
        (ss,) = R.adam_norms((4,), g, 1)
        assert not R.norm_fragile(ss, 4), k
        z = np.zeros(4, np.float32)
        assert R.adam_ref((4,), 1, 1, R.LR, R.MAX_NORM, R.ADAM_EPS, g, z, z, z)[3] == [want], k
        assert (np.float32(np.sqrt(ss)) == R.MAX_NORM) == (not want)


def _oracle_adam(desc, step, grad, params, m1, m2):
    nt = 2 * 4
    a = O.Adam()
    O.lib().or_adam_init(C.byref(a), C.byref(desc))
    try:
        n = desc.n_params
        C.memmove(a.m1, m1.ctypes.data, n * 4)
        C.memmove(a.m2, m2.ctypes.data, n * 4)
        for t in range(nt):
            a.time[t] = step - 1
        p = params.copy()
        O.lib().or_adam_step(C.byref(desc), C.byref(a), p, grad.copy(), float(R.LR), R.MAX_NORM, R.ADAM_EPS)
        return p, np.ctypeslib.as_array(a.m1, (n,)).copy(), np.ctypeslib.as_array(a.m2, (n,)).copy()
    finally:
        O.lib().or_adam_free(C.byref(a))


def test_adam_restatement_is_or_adam_step_bit_for_bit():
    """the CfgB net's tensors through every step of the chain (world = 2: the oracle gets the
    halved gradient, an exact scaling)"""
    desc = O.mlp_desc(5, 2, 64, 2)
    assert desc.n_params == sum(R.CFGB_TENSORS)
    for c in R.adam_chain("cfgB"):
        g = (c["grad"] * np.float32(1.0 / c["world"])).astype(np.float32)
        got = _oracle_adam(desc, c["step"], g, *c["before"])
        for a, b, what in zip(got, c["after"], ("params", "m1", "m2")):
            assert np.array_equal(R.bits(a), R.bits(b)), (c["step"], c["kind"], what)
