"""Stats-mode evaluation without a GPU: the reference's own known answers (eval.rs tests)
on three implementations -- the Python restatement (tests/eval_ref.py), the product's
host-side hooks bppo_debug_eval_perms and bppo_debug_eval_sample(device = 0) (the host
build of the source the HIP kernels compile), and bppo/eval.py -- then 4,096 random rows
of the sampler, exact."""
import ctypes as C

import numpy as np
import pytest

import eval_ref as R
from test_abi import _ctypes_struct, _header_struct, _rust_struct

f32 = np.float32


def hook_perms(n):
    import bppo._lib as L
    out = np.zeros((int(np.prod(range(1, n + 1))), n), np.int32)
    assert L.lib().bppo_debug_eval_perms(n, out.ctypes.data) == L.OK
    return out.tolist()


def hook_sample(A, logits, masks, temps, seed, word_pos, device=0, stream=0):
    """-> (actions, draws_used) of bppo_debug_eval_sample"""
    import bppo._lib as L
    logits = np.ascontiguousarray(logits, f32).reshape(-1, A)
    masks = np.ascontiguousarray(masks, np.uint8).reshape(-1, A)
    temps = np.ascontiguousarray(temps, f32)
    B = logits.shape[0]
    act = np.full(B, -1, np.int32)
    used = np.full(B, -1, np.int32)
    st = L.lib().bppo_debug_eval_sample(device, A, B, logits.ctypes.data, masks.ctypes.data, temps.ctypes.data,
                                        seed, stream, word_pos, act.ctypes.data, used.ctypes.data)
    assert st == L.OK, st
    return act, used


def hook_sample_padded(logits, mask, temp):
    """a short row on the 7-action hook: the extra actions masked (they become -inf, so
    they are neither maxima nor carry probability)"""
    n = len(logits)
    lg = np.zeros(7, f32); lg[:n] = logits
    mk = np.zeros(7, np.uint8); mk[:n] = [1] * n if mask is None else mask
    a, u = hook_sample(7, lg, mk, [temp], 42, 0)
    return int(a[0]), int(u[0])


# ------------------------------------------------------------ known answers ---
def _schedules():
    import bppo
    return [R.TempSchedule, bppo.TempSchedule]


@pytest.mark.parametrize("impl", [0, 1])
def test_temp_schedule_known_answers(impl):
    T = _schedules()[impl]
    s = T(0.5, 0.0, None, False)                       # test_temp_schedule_constant
    assert s.get_temp(0) == f32(0.5) and s.get_temp(100) == f32(0.5)
    s = T(1.0, 0.3, 10, False)                         # test_temp_schedule_hard_cutoff
    assert [s.get_temp(m) for m in (0, 9, 10, 100)] == [f32(1.0), f32(1.0), f32(0.3), f32(0.3)]
    s = T(1.0, 0.0, 10, True)                          # test_temp_schedule_decay
    assert s.get_temp(0) == f32(1.0) and abs(s.get_temp(5) - 0.5) < 0.01 and s.get_temp(10) == f32(0.0)
    s = T(1.0, 0.3, 0, False)                          # test_temp_schedule_cutoff_zero
    assert s.get_temp(0) == f32(0.3) and s.get_temp(100) == f32(0.3)
    # the decay is one fma of t = move / cutoff: t * (final - initial) + initial
    s = T(1.0, 0.2, 6, True)
    for m in range(6):
        t = f32(m) / f32(6)
        exact = f32(float(t) * float(f32(0.2) - f32(1.0)) + 1.0)   # f64: exact product, one rounding here
        assert s.get_temp(m) == exact


def test_temp_schedule_argument_errors_and_env_defaults():
    import bppo
    T = bppo.TempSchedule
    s = T.from_args("cartpole", temp=0.5)              # test_temp_schedule_from_args_valid
    assert s.get_temp(0) == f32(0.5) and s.get_temp(100) == f32(0.5)
    s = T.from_args("cartpole", temp=0.5, temp_cutoff=10, temp_final=0.1)
    assert s.get_temp(0) == f32(0.5) and s.get_temp(10) == f32(0.1)
    with pytest.raises(ValueError, match="--temp-final requires --temp-cutoff"):
        T.from_args("liars_dice", temp=0.5, temp_final=0.1)
    with pytest.raises(ValueError, match="--temp-decay requires --temp-cutoff"):
        T.from_args("liars_dice", temp=0.5, temp_decay=True)
    c4 = T.env_default("connect_four")                 # EVAL_TEMP 0.4, cutoff (10, 0.0)
    assert (c4.initial, c4.final_temp, c4.cutoff, c4.decay) == (f32(0.4), f32(0.0), 10, False)
    for env in ("liars_dice", "skull"):
        s = T.env_default(env)
        assert (s.initial, s.cutoff) == (f32(1.0), None)
    s = T.from_args("connect_four", no_temp_cutoff=True)
    assert s.cutoff is None and s.initial == f32(0.4)


def test_sample_known_answers():
    def never():
        raise AssertionError("temperature 0 must not draw")
    # test_sample_deterministic / test_sample_with_mask
    assert R.sample_with_temperature([1.0, 2.0, 0.5], None, 0.0, never) == (1, 0)
    assert R.sample_with_temperature([10.0, 2.0, 0.5], [False, True, True], 0.0, never) == (1, 0)
    assert hook_sample_padded([1.0, 2.0, 0.5], None, 0.0) == (1, 0)
    assert hook_sample_padded([10.0, 2.0, 0.5], [0, 1, 1], 0.0) == (1, 0)
    # test_sample_all_masked_fallback: NaN arithmetic, a draw is consumed, the last index
    words = iter(R.O.stdrng_words(42, 4))
    assert R.sample_with_temperature([1.0, 2.0, 3.0], [False] * 3, 1.0, lambda: next(words)) == (2, 1)
    a, u = hook_sample(7, np.arange(7, dtype=f32), np.zeros(7, np.uint8), [1.0], 42, 0)
    assert (int(a[0]), int(u[0])) == (6, 1)
    # the last of equal maxima at temperature 0
    assert R.sample_with_temperature([3.0, 1.0, 3.0], None, 0.0, never) == (2, 0)
    assert hook_sample_padded([3.0, 1.0, 3.0], None, 0.0) == (2, 0)


def test_rewards_to_placements_known_answers():
    import bppo
    for fn in (R.rewards_to_placements, bppo.rewards_to_placements):
        assert fn([1.0, 0.5, 0.0]) == [1, 2, 3]
        assert fn([0.0, 1.0, 0.5]) == [3, 1, 2]
        assert fn([1.0, 1.0]) == [1, 1]
        assert fn([1.0, 0.5, 0.5]) == [1, 2, 2]


def test_permutations_known_answers():
    import bppo
    for fn in (R.generate_permutations, bppo.generate_permutations, hook_perms):
        for n, count in ((2, 2), (3, 6), (4, 24)):
            perms = fn(n)
            assert len(perms) == count and len({tuple(p) for p in perms}) == count
            assert all(sorted(p) == list(range(n)) for p in perms)
        assert fn(2) == [[0, 1], [1, 0]]
        assert fn(3) == [[0, 1, 2], [1, 0, 2], [2, 0, 1], [0, 2, 1], [1, 2, 0], [2, 1, 0]]
    for n in (1, 5, 6):
        assert hook_perms(n) == R.generate_permutations(n)


# ------------------------------------------------------------- 4,096 rows ---
SAMPLER_SEED, SAMPLER_POS = 20260, 13      # the rows' words start mid-block


def sampler_rows(A, B, seed):
    """random rows: masks with at least one valid action, temps from {0, 0.05, 0.4, 1.0},
    logits x 20 at temp 0.05 (exp underflows to subnormals and zeros), tied maxima at temp 0"""
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((B, A)).astype(f32)
    masks = (rng.random((B, A)) < 0.6).astype(np.uint8)
    masks[np.arange(B), rng.integers(0, A, B)] = 1
    temps = rng.choice(np.array([0.0, 0.05, 0.4, 1.0], f32), B)
    logits[temps == f32(0.05)] *= f32(20.0)
    for b in np.nonzero(temps == 0.0)[0][::2]:          # every other argmax row: the maximum repeated
        valid = np.nonzero(masks[b])[0]
        top = logits[b, valid].max()
        logits[b, rng.choice(valid, min(3, len(valid)), replace=False)] = top
    return logits, masks, temps


_ref_cache = {}


def reference_rows(A, B, seed):
    """the Python sampler on sampler_rows, computed once per shape (shared with the GPU test)"""
    key = (A, B, seed)
    if key not in _ref_cache:
        logits, masks, temps = sampler_rows(A, B, seed)
        words = iter(R.O.stdrng_words(SAMPLER_SEED, B + 1, SAMPLER_POS))
        act = np.zeros(B, np.int32); used = np.zeros(B, np.int32)
        subnormal = 0
        for b in range(B):
            act[b], used[b] = R.sample_with_temperature(logits[b], masks[b], temps[b], lambda: next(words))
            if temps[b] == f32(0.05):
                x = np.where(masks[b] != 0, logits[b], -np.inf).astype(f32) / f32(0.05)
                e = np.exp((x - x.max()).astype(np.float64))
                subnormal += int(np.any((e > 0) & (e < 1.17549435e-38)))
        _ref_cache[key] = (logits, masks, temps, act, used, subnormal)
    return _ref_cache[key]


ROW_SHAPES = [(7, 1366, 1), (33, 1365, 2), (49, 1365, 3)]      # 4,096 rows in all


@pytest.mark.parametrize("A,B,seed", ROW_SHAPES)
def test_host_sampler_matches_python_on_random_rows(A, B, seed):
    logits, masks, temps, act, used, subnormal = reference_rows(A, B, seed)
    assert subnormal > 0, "the rows must reach subnormal exp results"
    assert 0 < used.sum() < B and np.array_equal(used, (temps != 0).astype(np.int32))
    a, u = hook_sample(A, logits, masks, temps, SAMPLER_SEED, SAMPLER_POS)
    assert np.array_equal(u, used)
    assert np.array_equal(a, act)


# ------------------------------------------------------------ struct sizes ---
@pytest.mark.parametrize("c_name,rust_name,attr,size_fn", [
    ("bppo_eval_config", "BppoEvalConfig", "EvalConfig", "bppo_eval_config_size"),
    ("bppo_eval_game", "BppoEvalGame", "EvalGame", "bppo_eval_game_size")])
def test_eval_struct_layouts(c_name, rust_name, attr, size_fn):
    import bppo._lib as L
    hdr = _header_struct(c_name)
    assert _ctypes_struct(getattr(L, attr)) == hdr
    assert _rust_struct(rust_name) == hdr
    assert getattr(L.lib(), size_fn)() == C.sizeof(getattr(L, attr))
    assert C.sizeof(L.EvalGame) == 64 and C.sizeof(L.EvalConfig) == 32


# ------------------------------------------- the restated loop on its own ---
def test_restated_loop_freeze_rule_connect_four():
    """N = 16, 5 games, temperature 0: the first freeze takes envs 0..10 by the index-order
    fallback, the five games come from envs 11..15, and only next_u64 touches the RNG"""
    d = R.O.mlp_desc(86, 7, 64, 2)
    import bppo
    cfg = bppo.make_config("connect_four", hidden_size=64, num_hidden=2)
    models = [R.Model(d, bppo.orthogonal_init(cfg, seed=1)), R.Model(d, bppo.orthogonal_init(cfg, seed=2))]
    out = R.run_stats_mode("connect_four", 16, 2, models, [0, 1], 5, R.TempSchedule(0.0), seed=7)
    assert out["ended_by"] == "num_games" and len(out["games"]) == 5
    assert sorted(g[3] for g in out["games"]) == [11, 12, 13, 14, 15]
    assert out["rng_pos"] == 2
