"""The return normalizer's kernels (k_rn_returns, k_rn_returns_mp<P>, k_rn_block_agg,
k_rn_agg_scan, k_rn_apply, k_rn_scatter_acting in k_gae.hip) on raw arrays through
bppo_debug_return_norm, against the plain f64 restatement in tests/ret_norm_ref.py (tied to
the oracle bit for bit by tests/test_ret_norm_ref.py).

Shapes follow the kernels' structure: the 16-step unrolled body of the per-env walk alone, its
tail alone and both (T = 16, 1 / 15, 17 / 33 / 40); partial waves and blocks (N = 1, 63, 64, 65,
300); the 4096-element scan segment at 4095, 4096, 4097 elements and three blocks with a ragged
last one; every player count 1..6 (P = 5 and 6 read and wrote player 3's return before
k_rn_returns_mp became a template over P).

Bars (the project's own, tests/test_gpu_wide.py): returns_state equal to the reference, the
count exactly equal, mean and m2 within rtol 1e-12 (the device merges Welford states block by
block, the reference pushes one sample at a time), rewards and all_rewards within rtol 2e-7 and
atol 0 (one f32 ulp where the two standard deviations differ in their last bits), elements left
before n >= 2 and the non-acting slots of all_rewards bit-equal to their inputs."""
import numpy as np
import pytest

import bppo._lib as L
from ret_norm_ref import fresh_state, make_inputs, return_norm_ref, seeded_state

pytestmark = pytest.mark.gpu
GAMMA = 0.99


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _hook(P, clip, inp, R0, st0, mp=True):
    """bppo_debug_return_norm on copies -> dict like return_norm_ref's.  mp=False: players NULL
    (k_rn_returns; P = 1, no valid, no all_rewards)"""
    T, N = inp["rew_raw"].shape
    R = np.ascontiguousarray(R0, np.float64).copy()
    st = np.ascontiguousarray(st0, np.float64).copy()
    rew = np.full((T, N), np.nan, np.float32)
    valid = inp["valid"] if mp else None
    allr = np.ascontiguousarray(inp["all_rewards"]).copy() if mp else None
    ptr = [None if a is None else a.ctypes.data
           for a in (inp["rew_raw"], inp["done"], inp["players"] if mp else None, valid, R, st, rew, allr)]
    assert R.shape == (N, P) and inp["rew_raw"].flags.c_contiguous and inp["done"].flags.c_contiguous
    assert inp["players"].flags.c_contiguous and inp["players"].dtype == np.int32
    assert valid is None or (valid.flags.c_contiguous and valid.dtype == np.float32)
    assert L.lib().bppo_debug_return_norm(T, N, P, GAMMA, clip, *ptr) == L.OK
    return dict(rew=rew, returns_state=R, stats3=st, all_rewards=allr)


def _ref(clip, inp, R0, st0, mp=True):
    return return_norm_ref(GAMMA, clip, inp["rew_raw"], inp["done"], inp["players"] if mp else None,
                           inp["valid"] if mp else None, R0, st0, inp["all_rewards"] if mp else None)


def _check(out, ref, inp):
    bad = np.argwhere(out["returns_state"] != ref["returns_state"])
    assert bad.size == 0, "returns_state differs in %d slots, players %s, first (env, player) %s" % (
        len(bad), sorted(set(bad[:, 1].tolist())), bad[0].tolist())
    assert not np.isnan(out["returns_state"]).any()
    assert out["stats3"][2] == ref["stats3"][2]
    np.testing.assert_allclose(out["stats3"], ref["stats3"], rtol=1e-12, atol=0)
    assert not np.isnan(out["rew"]).any()
    np.testing.assert_allclose(out["rew"], ref["rew"], rtol=2e-7, atol=0)
    raw = ~ref["normalized"]
    assert np.array_equal(_bits(out["rew"][raw]), _bits(inp["rew_raw"][raw]))
    if out["all_rewards"] is not None:
        np.testing.assert_allclose(out["all_rewards"], ref["all_rewards"], rtol=2e-7, atol=0)
        acting = np.zeros(ref["all_rewards"].shape, bool)
        np.put_along_axis(acting, inp["players"][..., None].astype(np.int64), True, axis=2)
        assert np.array_equal(_bits(out["all_rewards"][~acting]), _bits(inp["all_rewards"][~acting]))
        assert np.array_equal(_bits(out["all_rewards"][acting]), _bits(out["rew"].reshape(-1)))


def _same_bits(a, b):
    assert np.array_equal(_bits(a["rew"]), _bits(b["rew"]))
    assert np.array_equal(a["returns_state"].view(np.uint64), b["returns_state"].view(np.uint64))
    assert np.array_equal(a["stats3"].view(np.uint64), b["stats3"].view(np.uint64))


# T x N: body / tail of the 16-step unroll x partial waves and blocks; then the scan segment:
# 4095, 4096, 4097 elements, and 8481 = 2.07 x 4096 (three blocks, the last one ragged)
SHAPES = [(T, N) for T in (1, 15, 16, 17, 33, 40) for N in (1, 63, 64, 65, 300)] + [
    (1, 4095), (1, 4096), (17, 241), (33, 257)]
_FAM = [("sparse", "random"), ("dense", "step"), ("sparse", "none"), ("dense", "random"), ("sparse", "step")]


@pytest.mark.parametrize("T,N", SHAPES)
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 6])
def test_shapes_every_player_count(P, T, N):
    """seeded statistics and a non-zero return in every (env, player) slot"""
    k = SHAPES.index((T, N))
    rewards, dones = _FAM[(k + P) % len(_FAM)]
    inp = make_inputs(1000 * P + k, T, N, P, rewards, dones)
    R0, st0 = seeded_state(k, N, P)
    assert (R0 != 0).all()
    ref = _ref(10.0, inp, R0, st0)
    out = _hook(P, 10.0, inp, R0, st0)
    _check(out, ref, inp)
    if P == 1:                      # k_rn_returns and k_rn_returns_mp<1> agree bit for bit
        one = _hook(1, 10.0, inp, R0, st0, mp=False)
        _check(one, _ref(10.0, inp, R0, st0, mp=False), inp)
        _same_bits(one, out)


@pytest.mark.parametrize("dones", ["step", "none", "random"])
@pytest.mark.parametrize("P,mp,valid", [(1, False, None), (1, True, "random"), (3, True, None), (5, True, "random"),
                                        (6, True, None), (6, True, "random")])
def test_fresh_statistics_first_valid_element_leaves_raw(P, mp, valid, dones):
    T, N = 17, 65
    inp = make_inputs(77 + P, T, N, P, "sparse" if P % 2 else "dense", dones, valid)
    inp["rew_raw"][0, :4] = (0.33, -1.0, 1.0, 0.33)        # no zero where raw and normalized must differ
    R0, st0 = fresh_state(N, P)
    ref = _ref(10.0, inp, R0, st0, mp=mp)
    raw = ~ref["normalized"].reshape(-1)
    # n < 2 up to the row before the second valid one: the first valid element leaves raw
    first, second = (0, 1) if valid is None else (int(i) for i in np.flatnonzero(inp["valid"].reshape(-1) > 0.5)[:2])
    assert raw[:second].all() and not raw[second:].any() and first < second
    nz = inp["rew_raw"].reshape(-1) != 0
    assert (ref["rew"].reshape(-1)[second:][nz[second:]] != inp["rew_raw"].reshape(-1)[second:][nz[second:]]).all()
    out = _hook(P, 10.0, inp, R0, st0, mp=mp)
    assert np.array_equal(_bits(out["rew"].reshape(-1)[:second]), _bits(inp["rew_raw"].reshape(-1)[:second]))
    _check(out, ref, inp)


@pytest.mark.parametrize("P,mp", [(1, False), (1, True), (4, True), (5, True), (6, True)])
def test_chained_calls_equal_one_call(P, mp):
    """T1 = 17 then T2 = 16 steps fed the first call's state == one call over 33 steps
    (N = 300: 9900 elements, the split at element 5100 inside the second scan block)"""
    T1, T2, N = 17, 16, 300
    inp = make_inputs(500 + P, T1 + T2, N, P, "dense" if P % 2 else "sparse", "random", "random" if mp else None)
    R0, st0 = seeded_state(P, N, P)
    ref = _ref(10.0, inp, R0, st0, mp=mp)
    whole = _hook(P, 10.0, inp, R0, st0, mp=mp)
    _check(whole, ref, inp)

    def part(a, b):
        return {k: None if v is None else np.ascontiguousarray(v[a:b]) for k, v in inp.items()}
    one = _hook(P, 10.0, part(0, T1), R0, st0, mp=mp)
    _check(one, _ref(10.0, part(0, T1), R0, st0, mp=mp), part(0, T1))
    two = _hook(P, 10.0, part(T1, T1 + T2), one["returns_state"], one["stats3"], mp=mp)
    chained = dict(rew=np.concatenate([one["rew"], two["rew"]]), returns_state=two["returns_state"],
                   stats3=two["stats3"],
                   all_rewards=np.concatenate([one["all_rewards"], two["all_rewards"]]) if mp else None)
    _check(chained, ref, inp)
    assert np.array_equal(chained["returns_state"], whole["returns_state"])
    assert chained["stats3"][2] == whole["stats3"][2]
    np.testing.assert_allclose(chained["stats3"], whole["stats3"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(chained["rew"], whole["rew"], rtol=2e-7, atol=0)


@pytest.mark.parametrize("P", [1, 2, 5, 6])
@pytest.mark.parametrize("seeded", [False, True])
def test_valid_random_half(P, seeded):
    T, N = 33, 257
    inp = make_inputs(40 + P, T, N, P, "sparse", "random", "random")
    R0, st0 = seeded_state(P, N, P) if seeded else fresh_state(N, P)
    ref = _ref(10.0, inp, R0, st0)
    assert ref["stats3"][2] - st0[2] == (inp["valid"] > 0.5).sum() < T * N
    _check(_hook(P, 10.0, inp, R0, st0), ref, inp)


@pytest.mark.parametrize("P", [1, 4, 5, 6])
def test_first_scan_block_all_invalid(P):
    """the first 4133 rows invalid, fresh statistics: the whole first scan block contributes
    nothing, the count is below 2 up to row 4133 and those rewards pass through raw"""
    T, N, head = 33, 257, 4096 + 37
    inp = make_inputs(60 + P, T, N, P, "dense", "random", "head", head=head)
    R0, st0 = fresh_state(N, P)
    ref = _ref(10.0, inp, R0, st0)
    raw = ~ref["normalized"].reshape(-1)
    assert raw[:head + 1].all() and not raw[head + 1:].any() and ref["stats3"][2] == T * N - head
    out = _hook(P, 10.0, inp, R0, st0)
    assert np.array_equal(_bits(out["rew"].reshape(-1)[:head + 1]), _bits(inp["rew_raw"].reshape(-1)[:head + 1]))
    _check(out, ref, inp)


@pytest.mark.parametrize("P", [1, 3, 6])
@pytest.mark.parametrize("seeded", [False, True])
def test_all_rows_invalid_leaves_statistics(P, seeded):
    T, N = 17, 300
    inp = make_inputs(80 + P, T, N, P, "sparse", "random", "none")
    R0, st0 = seeded_state(P, N, P) if seeded else fresh_state(N, P)
    ref = _ref(10.0, inp, R0, st0)
    out = _hook(P, 10.0, inp, R0, st0)
    assert np.array_equal(out["stats3"].view(np.uint64), np.asarray(st0, np.float64).view(np.uint64))
    if not seeded:
        assert np.array_equal(_bits(out["rew"]), _bits(inp["rew_raw"]))            # n stays 0: every reward raw
    else:
        assert ref["normalized"].all() and (out["rew"] != inp["rew_raw"])[inp["rew_raw"] != 0].all()
    _check(out, ref, inp)                  # the rolling returns move all the same


@pytest.mark.parametrize("P", [1, 2, 5, 6])
def test_invalid_row_on_a_done_step_still_resets(P):
    """every done row invalid, and the last step all done and all invalid: the acting player's
    return ends the call at 0 although none of those rows entered the statistics"""
    T, N = 17, 65
    inp = make_inputs(90 + P, T, N, P, "dense", "step", "done")
    inp["done"][T - 1] = 1.0
    inp["valid"][T - 1] = 0.0
    assert not (inp["valid"][inp["done"] != 0] > 0.5).any()
    R0, st0 = seeded_state(P, N, P)
    ref = _ref(10.0, inp, R0, st0)
    out = _hook(P, 10.0, inp, R0, st0)
    last = inp["players"][T - 1]
    assert (out["returns_state"][np.arange(N), last] == 0.0).all()
    assert ref["stats3"][2] - st0[2] == (inp["valid"] > 0.5).sum()
    _check(out, ref, inp)


@pytest.mark.parametrize("P,mp", [(1, False), (2, True), (6, True)])
def test_clip_engages_both_clamps(P, mp):
    T, N = 40, 65
    inp = make_inputs(120 + P, T, N, P, "dense", "random")
    R0, st0 = seeded_state(P, N, P)
    ref = _ref(0.5, inp, R0, st0, mp=mp)
    c = ref["clamped"]
    assert (c == 1).sum() > 50 and (c == -1).sum() > 50 and (c == 0).sum() > 50     # not vacuous
    assert (ref["rew"][c == 1] == np.float32(0.5)).all() and (ref["rew"][c == -1] == np.float32(-0.5)).all()
    assert (np.abs(ref["rew"][c == 0]) <= np.float32(0.5)).all()
    _check(_hook(P, 0.5, inp, R0, st0, mp=mp), ref, inp)
