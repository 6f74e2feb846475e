"""The update's metric fold (csrc/bppo_update_metrics.h, through bppo_debug_fold_metrics)
against a numpy float32 restatement of ppo.rs:2025-2110 / oracle/ppo.c:700-745: every field of
bppo_update_metrics bit for bit, NaN matching NaN.  No HIP call: runs without a GPU.

A metric row is what one minibatch leaves on the device: WM_COUNT sums over its rows (slot
names as in csrc/bppo_wide.h) and its four raw-advantage statistics."""
import ctypes as C
import ctypes.util
import math

import numpy as np
import pytest

import bppo._lib as L

PL, VL, H, KL, CF, V, R, VE, VE2, VEMAX, N, VALID, HV, NCHOICE, COUNT = range(15)
ADV_MEAN, ADV_STD, ADV_MIN, ADV_MAX = range(COUNT, COUNT + 4)
WIDTH = COUNT + 4
ENV_CARTPOLE, ENV_CONNECT_FOUR = 0, 1
f32 = np.float32

_libm = C.CDLL(ctypes.util.find_library("m"))
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]


def _args(**kw):
    d = dict(value_coef=0.5, ent_coef=0.01, A=7, env_kind=ENV_CONNECT_FOUR, B=512, ev4=(0.0, 0.0, 0.0, 0.0),
             ev_mode=0, ev_ref=0.0, epochs_run=1, normalize_values=0, pa_tsum=0.0, pa_tsq=0.0, pa_tcount=0.0,
             pa_rescale_mag=0.0)
    d.update(kw)
    return d


def fold_ref(rows, a):
    """f32 operations in the reference's order; f64 where the reference widens"""
    rows = np.asarray(rows, f32).reshape(-1, WIDTH)
    vc, ec = f32(a["value_coef"]), f32(a["ent_coef"])
    z = f32(0)
    tp = tv = th = tk = tc = tl = tvm = trm = tam = tas = tvem = tves = tav = tevp = z
    tamin, tamax, tvemax = f32(np.inf), f32(-np.inf), f32(-np.inf)
    with np.errstate(all="ignore"):
        for r in rows:
            n = r[N] if r[N] > 0 else f32(1)
            pl, vl, h = r[PL] / n, f32(0.5) * (r[VL] / n), r[H] / n
            tp = tp + pl; tv = tv + vl; th = th + h; tk = tk + r[KL] / n; tc = tc + r[CF] / n
            tl = tl + ((pl + vl * vc) + (-h) * ec)
            tvm = tvm + r[V] / n; trm = trm + r[R] / n
            vem = r[VE] / n
            tvem = tvem + vem
            # the sample variance of (return - value) from its two sums, in f64 (n - 1 in f32)
            var = (float(r[VE2]) - float(n) * float(vem) * float(vem)) / float(n - f32(1)) if n > 1 else 0.0
            tves = tves + np.sqrt(f32(max(var, 0.0)))
            tvemax = max(tvemax, r[VEMAX])
            tav = tav + r[VALID] / n
            tevp = tevp + (r[HV] / r[NCHOICE] if r[NCHOICE] > 0 else z)
            tam = tam + r[ADV_MEAN]; tas = tas + r[ADV_STD]
            tamin = min(tamin, r[ADV_MIN]); tamax = max(tamax, r[ADV_MAX])
        nup = len(rows)
        n = f32(nup)
        m = dict(policy_loss=tp / n, value_loss=tv / n, entropy=th / n, approx_kl=tk / n, clip_fraction=tc / n,
                 total_loss=tl / n, value_mean=tvm / n, returns_mean=trm / n, adv_mean_raw=tam / n,
                 adv_std_raw=tas / n, adv_min_raw=tamin, adv_max_raw=tamax, value_error_mean=tvem / n,
                 value_error_std=tves / n, value_error_max=tvemax)
        m["entropy_scaled"] = m["entropy"] / f32(_libm.logf(float(a["A"])))
        masked = a["env_kind"] != ENV_CARTPOLE           # ppo.rs:1549-1565: None -> 0 without action masks
        m["avg_valid_actions"] = tav / n if masked else z
        m["entropy_valid_pct"] = tevp / n if masked else z
        # ppo.rs:1268-1294 from f64 sums: fewer than 2 rows or Var(R) < 1e-8 -> 0
        B = float(a["B"])
        s = [float(x) for x in a["ev4"]]
        mr = np.float64(s[0]) / B; vr = np.float64(s[1]) / B - mr * mr
        mres = np.float64(s[2]) / B; vres = np.float64(s[3]) / B - mres * mres
        m["explained_variance"] = z if (a["B"] < 2 or vr < 1e-8) else f32(1.0 - vres / vr)
        if a["ev_mode"] == 1:
            m["explained_variance"] = f32(a["ev_ref"])
        # PopArt (ppo.rs:2061-2068): None -> NaN
        m["value_norm_target_mean"] = m["value_norm_target_std"] = f32(np.nan)
        m["value_norm_rescale_mag"] = f32(a["pa_rescale_mag"])
        if a["normalize_values"] and a["pa_tcount"] > 0:
            mean = a["pa_tsum"] / a["pa_tcount"]
            var = a["pa_tsq"] / a["pa_tcount"] - mean * mean
            m["value_norm_target_mean"] = f32(mean)
            m["value_norm_target_std"] = f32(math.sqrt(max(var, 0.0)))
    m["num_updates"], m["epochs_run"] = nup, a["epochs_run"]
    return m


def fold_dev(rows, a):
    rows = np.ascontiguousarray(rows, f32).reshape(-1, WIDTH)
    fa = L.FoldArgs(**{k: v for k, v in a.items() if k != "ev4"})
    fa.ev4 = (C.c_double * 4)(*a["ev4"])
    out = L.UpdateMetrics()
    st = L.lib().bppo_debug_fold_metrics(rows.ctypes.data if len(rows) else None, len(rows), C.byref(fa), C.byref(out))
    assert st == L.OK
    return out


def check(rows, a):
    ref, out = fold_ref(rows, a), fold_dev(rows, a)
    for k in L.METRIC_NAMES + L.POPART_METRICS:
        got, want = f32(getattr(out, k)), f32(ref[k])
        assert got.view(np.uint32) == want.view(np.uint32), (k, got, want)
    assert (out.num_updates, out.epochs_run) == (ref["num_updates"], ref["epochs_run"])
    return out


def random_rows(nup, seed, n_rows=171, A=7):
    g = np.random.default_rng(seed)
    rows = np.zeros((nup, WIDTH), f32)
    for r in rows:
        n = float(n_rows + g.integers(0, 2))
        vem, sd = g.normal() * 0.3, abs(g.normal()) + 0.1
        r[[PL, VL, H, KL, CF]] = [g.normal() * n * 0.1, g.random() * n, g.random() * n * 1.9, g.random() * n * 0.02,
                                  float(g.integers(0, int(n)))]
        r[[V, R, VE, VE2, VEMAX, N]] = [g.normal() * n, g.normal() * n, vem * n, n * (vem * vem + sd * sd),
                                        abs(vem) + 3 * sd, n]
        nch = float(g.integers(1, int(n)))
        r[[VALID, HV, NCHOICE]] = [n * (1 + g.random() * (A - 1)), nch * g.random(), nch]
        r[[ADV_MEAN, ADV_STD, ADV_MIN, ADV_MAX]] = [g.normal() * 0.1, 1 + g.random(), -3 - g.random(), 3 + g.random()]
    return rows


def ev_sums(seed, B):
    g = np.random.default_rng(seed)
    ret, val = g.normal(size=B), g.normal(size=B)
    return (ret.sum(), (ret * ret).sum(), (ret - val).sum(), ((ret - val) ** 2).sum())


@pytest.mark.parametrize("nup", [1, 3, 24])
def test_seeded_random_rows(nup):
    out = check(random_rows(nup, seed=nup), _args(B=512, ev4=ev_sums(nup, 512), epochs_run=2))
    assert out.num_updates == nup and np.isfinite(out.total_loss) and out.explained_variance != 0.0


def test_no_minibatch_ran():
    out = check(np.zeros((0, WIDTH), f32), _args(B=0, epochs_run=3))
    for k in ("policy_loss", "value_loss", "entropy", "approx_kl", "total_loss", "adv_mean_raw", "value_error_std"):
        assert math.isnan(getattr(out, k)), k
    assert out.adv_min_raw == math.inf and out.adv_max_raw == -math.inf and out.value_error_max == -math.inf
    assert out.num_updates == 0 and out.epochs_run == 3


def test_lockstep_empty_slot():
    """W > 1: a slot without rows on this rank leaves zero sums, value_error_max -inf and zero
    advantage statistics; it still counts as an update"""
    rows = random_rows(3, seed=11)
    rows[1] = 0.0
    rows[1, VEMAX] = -np.inf
    out = check(rows, _args())
    assert out.num_updates == 3 and np.isfinite(out.value_error_max)
    only = np.zeros((1, WIDTH), f32)
    only[0, VEMAX] = -np.inf
    out = check(only, _args())
    assert out.policy_loss == 0.0 and out.value_error_max == -math.inf and out.adv_min_raw == 0.0


def test_single_row_minibatch_has_zero_error_std():
    rows = random_rows(1, seed=5)
    rows[0, N] = 1.0
    assert check(rows, _args()).value_error_std == 0.0
    rows = random_rows(2, seed=6)
    rows[1, N] = 1.0
    check(rows, _args())


def test_no_row_with_a_choice():
    rows = random_rows(2, seed=7)
    rows[0, NCHOICE] = 0.0
    check(rows, _args())
    rows[1, NCHOICE] = 0.0
    assert check(rows, _args()).entropy_valid_pct == 0.0


def test_cartpole_reports_no_mask_metrics():
    rows = random_rows(3, seed=8, A=2)
    cp = check(rows, _args(env_kind=ENV_CARTPOLE, A=2))
    assert cp.avg_valid_actions == 0.0 and cp.entropy_valid_pct == 0.0
    c4 = check(rows, _args(env_kind=ENV_CONNECT_FOUR, A=2))
    assert c4.avg_valid_actions > 0.0 and c4.entropy_valid_pct > 0.0
    assert cp.entropy_scaled == c4.entropy_scaled


def test_explained_variance_degenerate_and_reference_mode():
    rows = random_rows(2, seed=9)
    assert check(rows, _args(B=1, ev4=(2.0, 4.0, 0.5, 0.25))).explained_variance == 0.0
    assert check(rows, _args(B=0)).explained_variance == 0.0
    # Var(R) = 1e-9 < 1e-8: constant returns up to noise
    B, mean = 100, 3.0
    assert check(rows, _args(B=B, ev4=(B * mean, B * (mean * mean + 1e-9), 1.0, 5.0))).explained_variance == 0.0
    out = check(rows, _args(B=B, ev4=(B * mean, B * (mean * mean + 2.0), 10.0, 51.0)))
    assert 0.0 < out.explained_variance < 1.0
    # mode 1 reports the host thread's value whatever the sums say
    out = check(rows, _args(B=B, ev4=(B * mean, B * (mean * mean + 2.0), 10.0, 51.0), ev_mode=1, ev_ref=-0.375))
    assert out.explained_variance == -0.375


def test_popart_target_statistics():
    rows = random_rows(2, seed=10)
    on = check(rows, _args(normalize_values=1, pa_tsum=12.5, pa_tsq=400.0, pa_tcount=64.0, pa_rescale_mag=0.25))
    assert np.isfinite(on.value_norm_target_mean) and on.value_norm_target_std > 0 and on.value_norm_rescale_mag == 0.25
    # the variance's cancellation may go below zero: clamped
    assert check(rows, _args(normalize_values=1, pa_tsum=3.0, pa_tsq=0.9 - 1e-12, pa_tcount=10.0)).value_norm_target_std == 0.0
    for a in (_args(normalize_values=0, pa_tsum=12.5, pa_tsq=400.0, pa_tcount=64.0),
              _args(normalize_values=1, pa_tcount=0.0, pa_rescale_mag=0.5)):
        off = check(rows, a)
        assert math.isnan(off.value_norm_target_mean) and math.isnan(off.value_norm_target_std)


def test_rejects_missing_arguments():
    fa, out = L.FoldArgs(), L.UpdateMetrics()
    rows = np.zeros((1, WIDTH), f32)
    lib = L.lib()
    assert lib.bppo_debug_fold_metrics(rows.ctypes.data, 1, None, C.byref(out)) == L.ERR_ARG
    assert lib.bppo_debug_fold_metrics(rows.ctypes.data, 1, C.byref(fa), None) == L.ERR_ARG
    assert lib.bppo_debug_fold_metrics(None, 1, C.byref(fa), C.byref(out)) == L.ERR_ARG
    assert lib.bppo_debug_fold_metrics(rows.ctypes.data, -1, C.byref(fa), C.byref(out)) == L.ERR_ARG
