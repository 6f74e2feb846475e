"""The update's small kernels alone (k_update.hip), through their parity hooks, against exact
arithmetic on the f32 inputs (tests/update_kernels_ref.py states the rule, its case tables and
seeds; tests/test_update_kernels_ref.py settles the fragile-output caps without a GPU):

  bppo_debug_adv_stats    k_adv_epoch + k_adv_epoch_final, k_adv_stream<4|8|16> + k_adv_stream_final
  bppo_debug_slab_reduce  k_slab_reduce1
  bppo_debug_adam         k_adam_norm + k_adam + k_metric_row, and the fused k_adam1

min / max, the slab's max column and everything the Adam step writes: bit for bit.  Means and
column sums: bit for bit unless fragile, then within one ulp, at most max(1, outputs / 1000)
fragile outputs per case.  std: |std - ref| <= ref 0.5 kappa n 2^-53 + 1.5 ulp(ref), kappa =
sum a^2 / sum (a - mean)^2 (the device's one-pass f64 form against the oracle's two-pass one)."""
import ctypes as C
import math

import numpy as np
import pytest

import bppo._lib as L
import update_kernels_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32


# ====================================================== advantage statistics ==
def _adv_hook(B, M, adv, perm, inv):
    stats = np.full((M, 4), 12345.0, F32)
    path = C.c_int32(-1)
    st = L.lib().bppo_debug_adv_stats(B, M, adv.ctypes.data, perm.ctypes.data, None if inv is None else inv.ctypes.data,
                                      stats.ctypes.data, C.byref(path))
    assert st == L.OK, st
    return stats, path.value


_adv_seen_paths = set()
_adv_worst = {}


@pytest.mark.parametrize("B,M", R.ADV_CASES)
def test_adv_stats(B, M):
    for kind in R.adv_kinds(B):
        adv, perm, inv = R.adv_inputs(B, M, kind)
        ref = R.adv_reference(B, M, kind)
        for use_inv in (True, False):
            stats, path = _adv_hook(B, M, adv, perm, inv if use_inv else None)
            want_path = R.adv_plan(B, M, use_inv)[0]
            assert path == want_path and (path == 0 if (M > 16 or not use_inv or B < M) else path in (4, 8, 16))
            _adv_seen_paths.add(path)
            what = (B, M, kind, path)
            n_frag = 0
            for m, r in enumerate(ref):
                mean, std, mn, mx = stats[m]
                if r["n"] == 0:         # as or_normalize_advantages on no rows
                    assert np.isnan(mean) and np.isnan(std) and mn == np.inf and mx == -np.inf, (what, m, stats[m])
                    continue
                if r["n"] == 1 or kind == "equal":
                    assert R.bits(mn) == R.bits(r["min"]) and R.bits(mx) == R.bits(r["max"]), (what, m, mn, mx, r)
                    n_frag += R.check_outputs([mean], [r["mean"]], [r["mabs"]], r["n"], (what, m, "mean"))
                if r["n"] == 1:
                    assert np.isnan(std), (what, m, std)
                elif kind == "equal":
                    a = float(R.EQUAL_VALUE)
                    assert 0.0 <= std <= 2.0 ** -26 * a * math.sqrt(r["n"]), (what, m, std)
                    x = adv[:1]
                    assert ((x - mean) / (std + F32(1e-8)))[0] == 0.0, (what, m, mean, std)
                else:
                    frag, ratio = R.check_adv_stats(stats[m], r, (what, m))
                    n_frag += frag
                    k = "stream" if path else "perm"
                    _adv_worst[k] = max(_adv_worst.get(k, 0.0), ratio)
            assert n_frag <= R.fragile_cap(M), (what, n_frag)
    print(f"\nadv stats B={B} M={M}: worst std error / bound so far {_adv_worst}")


def test_adv_stats_reaches_every_kernel():
    """path_out names the kernel the launcher chose: 4 / 8 / 16 bins over the inverse, 0 over
    the permutation (no inverse, M > 16, B < M)"""
    got = {}
    for B, M in ((1000, 3), (1000, 8), (1000, 12), (1000, 17), (5, 8)):
        adv, perm, inv = R.adv_inputs(B, M, "n01")
        got[(B, M)] = (_adv_hook(B, M, adv, perm, inv)[1], _adv_hook(B, M, adv, perm, None)[1])
    assert got == {(1000, 3): (4, 0), (1000, 8): (8, 0), (1000, 12): (16, 0), (1000, 17): (0, 0), (5, 8): (0, 0)}
    if _adv_seen_paths:      # after the cases above
        assert _adv_seen_paths == {0, 4, 8, 16}
        print(f"\nadv stats: worst std error / bound per path {_adv_worst}")


# ============================================================ slab reduction ==
@pytest.mark.parametrize("rows,width", R.SLAB_CASES)
def test_slab_reduce(rows, width):
    exact, sabs = R.slab_reference(rows, width)
    col = width - R.NUM_M + R.M_VEMAX
    for max_row in sorted({rows - 1, 0}):       # the last row of the last non-empty group; row 0
        slab = R.slab_inputs(rows, width, max_row)
        out = np.full(width + R.SLAB_GUARD, np.nan, F32)
        guard = np.arange(R.SLAB_GUARD, dtype=F32) + F32(0.5)
        out[width:] = guard
        vemax = np.full(1, -1.0, F32)
        assert L.lib().bppo_debug_slab_reduce(rows, width, slab.ctypes.data, out.ctypes.data, vemax.ctypes.data) == L.OK
        assert not np.isnan(out[:width]).any(), np.flatnonzero(np.isnan(out[:width]))     # every column written
        assert np.array_equal(R.bits(out[width:]), R.bits(guard))                          # nothing behind them
        assert R.bits(out[col]) == R.bits(R.SLAB_MAX) == R.bits(vemax[0]), (max_row, out[col], vemax)
        assert rows == 1 or slab[:, col].sum() > 2 * R.SLAB_MAX                            # a sum would differ
        sums = np.delete(np.arange(width), col)
        n_frag = R.check_outputs(out[sums], exact[sums], sabs[sums], rows, (rows, width, max_row))
        assert n_frag <= R.fragile_cap(width), n_frag


# =============================================================== clip + Adam ==
GTAIL = (np.arange(R.GRAD_METRIC_SLOTS + 1, dtype=F32) + F32(1.25)) * F32(3.0)
MB_STATS = np.array([-0.5, 0.75, -7.0, 9.0], F32)


def _adam_hook(lens, step, world, fused, grad, params, m1, m2, max_norm=R.MAX_NORM):
    p, a, b = (np.array(x, F32) for x in (params, m1, m2))
    nm = R.GRAD_METRIC_SLOTS
    row = np.full(nm + 4, np.nan, F32)
    tl = np.array(lens, np.int32)
    st = L.lib().bppo_debug_adam(len(lens), tl.ctypes.data, step, world, R.LR, max_norm, R.ADAM_EPS, int(fused),
                                 np.ascontiguousarray(grad, F32).ctypes.data, p.ctypes.data, a.ctypes.data,
                                 b.ctypes.data, GTAIL.ctypes.data, MB_STATS.ctypes.data, nm, row.ctypes.data)
    assert st == L.OK, st
    return p, a, b, row


def _check_row(row):
    want = GTAIL[:R.GRAD_METRIC_SLOTS].copy()
    want[R.GRAD_VEMAX] = GTAIL[R.GRAD_VEMAX_LOCAL]
    assert np.array_equal(R.bits(row), R.bits(np.concatenate([want, MB_STATS]))), row


def _same(got, want, what):
    for g, w, name in zip(got, want, ("params", "m1", "m2")):
        bad = np.flatnonzero(R.bits(g) != R.bits(w))
        assert bad.size == 0, (what, name, bad.size, bad[:4], g[bad[:4]], w[bad[:4]])


@pytest.mark.parametrize("name", list(R.ADAM_TABLES))
def test_adam_matches_the_oracles_step_bit_for_bit(name):
    lens = R.ADAM_TABLES[name]
    can_fuse = max(lens) <= R.ADAM_CHUNK
    for c in R.adam_chain(name):
        what = (name, c["step"], c["kind"], c["world"])
        two = _adam_hook(lens, c["step"], c["world"], 0, c["grad"], *c["before"])
        _same(two[:3], c["after"], what + ("two-pass",))
        _check_row(two[3])
        if can_fuse:
            one = _adam_hook(lens, c["step"], c["world"], 1, c["grad"], *c["before"])
            _same(one[:3], c["after"], what + ("fused",))
            _same(one[:3], two[:3], what + ("fused vs two-pass",))
            assert np.array_equal(R.bits(one[3]), R.bits(two[3]))


def test_adam_clip_threshold():
    """norm == max_norm is not clipped (the comparison is >), also where one entry's extra ulp is
    rounded away in the f32 norm; three ulps make the norm the next float and clip"""
    z = np.zeros(4, F32)
    p0 = np.array([0.5, -0.25, 0.125, 1.0], F32)
    for k, g, want in R.threshold_cases():
        ref = R.adam_ref((4,), 1, 1, R.LR, R.MAX_NORM, R.ADAM_EPS, g, p0, z, z)
        assert ref[3] == [want]
        unclipped_m1 = g * F32(F32(1.0) - F32(0.9))
        assert np.array_equal(R.bits(ref[1]), R.bits(unclipped_m1)) == (not want)
        for fused in (0, 1):
            got = _adam_hook((4,), 1, 1, fused, g, p0, z, z)
            _same(got[:3], ref[:3], (k, fused))
