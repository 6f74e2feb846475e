"""What tests/test_gpu_loss_rows.py relies on, settled without a GPU (tests/loss_rows_ref.py holds
the rule, the seeds and the case tables):

  (a) or_loss_rows is the row loop of or_minibatch_loss_grad: its per-row terms, summed in row
      order, give or_mb_stats bit for bit;
  (b) its hand-written backward against torch f64 autograd of the loss expression of
      tests/test_oracle_backward.py, row by row, on the interior rows of every case;
  (c) the crafted rows land where intended: exact ratios bit for bit, and the whole truth table
      (placement x sign of A_n) -> (take_rhs, ratio in range, gradient passes), with at least 16
      rows of every category in the cases of 1000 rows and more;
  (d) every case stays inside the fragile-output cap of its metric sums."""
import ctypes as C
import re
import os

import numpy as np
import pytest
import torch

import loss_rows_ref as R
import oracle_ffi as O
import update_kernels_ref as U

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_sources_own():
    hdr = open(os.path.join(ROOT, "burn-ppo_amd", "csrc", "bppo_metric_row.h")).read()
    slots = re.search(r"enum \{ (WM_PL = 0[^}]*) \};", hdr).group(1).replace(" = 0", "").replace("\n", " ").split(",")
    slots = [s.strip()[3:] for s in slots]
    assert slots[:R.WM_COUNT] == sorted(R.WM, key=R.WM.get) and slots[R.WM_COUNT] == "COUNT"
    oh = open(os.path.join(ROOT, "oracle", "oracle.h")).read()
    terms = re.search(r"enum \{ (OR_LT_PL = 0[^}]*) \};", oh).group(1).replace(" = 0", "").replace("\n", " ").split(",")
    terms = [s.strip()[6:] for s in terms]
    assert terms[:R.LT_COUNT] == sorted(R.LT, key=R.LT.get) and terms[R.LT_COUNT] == "COUNT"
    assert U.GRAD_METRIC_SLOTS == R.WM_COUNT and U.GRAD_VEMAX_LOCAL == R.VEMAX_LOCAL and U.GRAD_VEMAX == R.WM["VEMAX"]
    src = open(os.path.join(ROOT, "burn-ppo_amd", "csrc", "bppo_wide.h")).read()
    assert "std::max(1, std::min(1024, (int)((mb + 255) / 256)))" in src      # GRID_N's second round
    for f in ("wide_api.hip", "k_wide.hip"):                                   # update and hook share the rule
        txt = open(os.path.join(ROOT, "burn-ppo_amd", "csrc", f)).read()
        assert "wide_loss_blocks(" in txt and "g.set_scalars(" in txt, f
    assert R.GRID_N > 1024 * 256


def test_case_table_covers_the_issue():
    ns = {c[0] for c in R.SHAPE_CASES}
    assert {1, 63, 64, 65, 255, 256, 257, 1000, R.GRID_N} <= ns
    assert any(c[1] > 0 for c in R.SHAPE_CASES) and {c[2] for c in R.SHAPE_CASES} == {0, 1}
    assert any("std0" in c[3] for c in R.SHAPE_CASES) and any("ones" in c[3] for c in R.SHAPE_CASES)
    assert [A for A in R.ACTION_COUNTS if any(R.SHAPE_CASES[k][0] == R.GRID_N for k in R.cases(A))] == [2, 7]
    assert any("ones" in R.SHAPE_CASES[k][3] for k in R.cases(2))


# ------------------------------------------------------------------ (a) refactor --
def _seq_sum(x):
    return float(np.cumsum(np.asarray(x, np.float64))[-1])        # one f64 add per row, in row order


@pytest.mark.parametrize("A,masked,clip_value,mb", [(2, False, False, 257), (7, True, True, 129), (49, True, False, 65)])
def test_loss_rows_summed_is_or_minibatch_loss_grad(A, masked, clip_value, mb):
    desc = O.mlp_desc(11, A, 32, 2)
    rng = np.random.default_rng([A, mb])
    params = (rng.normal(size=desc.n_params) * 0.3).astype(F32)
    obs = rng.normal(size=(mb, 11)).astype(F32)
    mk = None
    if masked:
        mk = (rng.random((mb, A)) < 0.6).astype(F32)
        mk[np.arange(mb), rng.integers(0, A, mb)] = 1.0
        mk[:5] = 0.0
        mk[:5, 2] = 1.0                                             # rows with one legal action
    act = np.array([rng.choice(np.flatnonzero(mk[i])) if masked else rng.integers(0, A) for i in range(mb)], np.int32)
    olp = (rng.normal(size=mb) * 0.3 - 1.0).astype(F32)
    adv, ret, ov = (rng.normal(size=mb).astype(F32) for _ in range(3))
    pc = O.ppo_cfg(clip=R.EPS, value_coef=R.VALUE_COEF, clip_value=clip_value)
    st = O.MbStats()
    grads = np.zeros(desc.n_params, F32)
    O.lib().or_minibatch_loss_grad(C.byref(desc), params, mb, obs, None, act, olp, adv, ret, ov,
                                   None if mk is None else mk.ctypes.data, C.byref(pc), R.ENT_COEF, grads, C.byref(st))
    logits, values = O.net_forward(desc, params, obs)
    _, _, t, _ = R.oracle_rows(A, mb, logits, values, act, olp, adv, ret, ov, mk, clip_value)
    inv = 1.0 / mb
    mean = lambda col: F32(_seq_sum(col) * inv)
    pl, h = mean(t[:, R.LT["PL"]]), mean(t[:, R.LT["H"]])
    vl = F32(mean(t[:, R.LT["VL"]]) * F32(0.5))
    vem = mean(t[:, R.LT["VE"]])
    dd = t[:, R.LT["VE"]].astype(np.float64) - float(vem)
    choice = t[:, R.LT["NVALID"]] > 1
    want = dict(
        loss=F32(F32(pl + F32(vl * F32(R.VALUE_COEF))) + F32(F32(-h) * F32(R.ENT_COEF))), policy_loss=pl, value_loss=vl,
        entropy=h, approx_kl=mean(t[:, R.LT["KL"]]), clip_fraction=mean(t[:, R.LT["CF"]]), value_mean=mean(values),
        returns_mean=mean(ret), value_error_mean=vem, value_error_std=np.sqrt(F32(_seq_sum(dd * dd) / (mb - 1))),
        value_error_max=t[:, R.LT["VE"]].max(),
        avg_valid_actions=mean(t[:, R.LT["NVALID"]]) if masked else F32(0),
        entropy_valid_pct=F32(_seq_sum(t[choice, R.LT["HV"]]) / choice.sum()) if masked else F32(0))
    for name, w in want.items():
        assert U.bits(getattr(st, name)) == U.bits(w), (name, getattr(st, name), w)
    if masked:
        assert (t[:5, R.LT["NVALID"]] == 1).all() and (t[:5, R.LT["H"]] == 0).all() and (t[:5, R.LT["HV"]] == 0).all()


# ------------------------------------------------------- (b) f64 autograd per row --
def _torch_rows(A, logits, values, act, olp, adv_n, ret, old_val, mask, clip_value):
    """d(row loss)/d(logits, value) of every row in f64: the expression of test_oracle_backward's
    _loss_tail without the mean over rows (mb = 1)"""
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    lg = t(logits).requires_grad_(True)
    v = t(values).requires_grad_(True)
    ls = torch.log_softmax(lg + (t(mask) - 1.0) * 1e9, 1)
    newlp = ls.gather(1, torch.tensor(act, dtype=torch.long)[:, None])[:, 0]
    H = -(ls.exp() * ls).sum(1)
    ratio = torch.exp(newlp - t(olp))
    na = -t(adv_n)
    pl = torch.maximum(na * ratio, na * ratio.clamp(1 - R.EPS, 1 + R.EPS))
    if clip_value:
        vo = t(old_val)
        vl = torch.maximum((v - t(ret)) ** 2, (vo + (v - vo).clamp(-R.EPS, R.EPS) - t(ret)) ** 2) * 0.5
    else:
        vl = ((v - t(ret)) ** 2) * 0.5
    (pl + vl * R.VALUE_COEF - H * R.ENT_COEF).sum().backward()
    # the magnitudes an entry is a difference of (loss_rows_ref.py, AUTOGRAD_*): |A_n| ratio of the
    # policy term (onehot against p), ent_coef p_a max(|ls_a|, H) of the entropy term (ls_a against -H)
    pol = (na.abs() * ratio).detach().numpy()
    ent = (R.ENT_COEF * (ls.exp() * torch.maximum(ls.abs(), H[:, None])).max(1).values).detach().numpy()
    return np.concatenate([lg.grad.numpy(), v.grad.numpy()[:, None]], axis=1), pol, ent


_autograd_worst = {}


@pytest.mark.parametrize("A", R.ACTION_COUNTS)
def test_oracle_backward_per_row_against_f64_autograd(A):
    worst, rows = 0.0, 0
    for k in R.cases(A):
        c, ref = R.case_inputs(A, k), R.case_reference(A, k)
        i = c["idx"]
        ok = R.interior(ref["terms"], c["clip_value"])
        g, pol, ent = _torch_rows(A, c["logits_mb"][ok], c["values_mb"][ok], c["act"][i][ok], c["logp"][i][ok],
                                  c["adv_n"][i][ok], c["ret"][i][ok], c["val"][i][ok], c["mask"][i][ok], c["clip_value"])
        got = ref["dout"][ok].astype(np.float64) * c["n"]
        passes = (ref["dec"][ok, 0] == 0) | (ref["dec"][ok, 1] == 1)
        scale = np.maximum(np.abs(g).max(axis=1), np.maximum(pol * passes, ent))
        # left out: a row with nothing to differentiate (one legal action, the value gradient cut),
        # one whose terms all lie in f32's denormal range (probabilities that underflowed), and one
        # below the f64 reference's own noise: autograd's log-softmax backward cancels terms of
        # size ent_coef to 2^-53, which a scale under ent_coef 2^-29 does not hide at 2^-24
        tiny = (scale / c["n"] < 2.0 ** -100) | (scale < R.ENT_COEF * 2.0 ** -29)
        assert tiny.sum() <= 0.2 * ok.sum() + 1 and (np.abs(got - g)[tiny] < R.ENT_COEF * 2.0 ** -29).all(), k
        err = np.abs(got - g)[~tiny].max(axis=1) / scale[~tiny]
        worst, rows = max(worst, float(err.max(initial=0.0))), rows + int(ok.sum())
        if c["n"] >= 1000:          # with clip_value the v == v_old ties, half of the rows, are left out too
            assert 0.1 * c["n"] < ok.sum() < c["n"], (k, ok.sum())
    _autograd_worst[A] = worst
    print(f"\nor_loss_rows vs f64 autograd, A = {A}: worst row error / scale {worst:.3e} over {rows} rows")
    assert R.AUTOGRAD_BAR[A] == 4 * R.AUTOGRAD_WORST[A] and R.AUTOGRAD_BAR[A] < 1e-4
    assert worst <= R.AUTOGRAD_BAR[A], (A, worst)


# ------------------------------------------------------ (c) crafted rows land --
@pytest.mark.parametrize("A,k", R.ALL_CASES)
def test_crafted_rows_land_where_intended(A, k):
    c, ref = R.case_inputs(A, k), R.case_reference(A, k)
    i, dec, t = c["idx"], ref["dec"], ref["terms"]
    pol, crafted = c["policy"][i], c["crafted"][i]
    ratio, adv_n = t[:, R.LT["RATIO"]], c["adv_n"][i]
    assert np.isfinite(ref["dout"]).all() and np.isfinite(t).all()
    big = c["n"] >= 1000
    if big:         # the search succeeds (the taken action's probability is chosen for it)
        assert crafted.mean() >= 0.99
    for j, (place, sign) in enumerate(R.POLICY):
        sel = (pol == j) & crafted
        if big:
            assert sel.sum() >= R.MIN_PER_CATEGORY, (place, sign, sel.sum())
        assert (np.sign(adv_n[sel]) == sign).all() and not np.signbit(adv_n[sel][adv_n[sel] == 0]).any()
        if place in R.TARGET:
            assert (U.bits(ratio[sel]) == U.bits(R.TARGET[place])).all(), (place, sign)
        elif place == "one":
            assert (ratio[sel] == 1.0).all() and (t[sel, R.LT["KL"]] == 0).all()
        elif place == "far_hi":
            assert (ratio[sel] > 2e4).all()
        elif place == "far_lo":
            assert (ratio[sel] < 5e-5).all()
        else:
            assert ((ratio[sel] > 0.85) & (ratio[sel] < 1.17)).all()
        rhs, inr, passes = R.TRUTH[(place, sign)]
        assert (dec[sel, 0] == rhs).all() and (dec[sel, 1] == inr).all(), (place, sign)
        # "passes" from the gradient itself: with the entropy term off, a cut row has dlogits == 0
        dl0, _, _, _ = R.oracle_rows(A, int(sel.sum()), c["logits_mb"][sel], c["values_mb"][sel], c["act"][i][sel],
                                     c["logp"][i][sel], adv_n[sel], c["ret"][i][sel], c["val"][i][sel],
                                     c["mask"][i][sel], c["clip_value"], ent=0.0) if sel.any() else (np.zeros((0, A)),) * 4
        moved = np.abs(dl0).max(axis=1) > 0 if sel.any() else np.zeros(0, bool)
        one_legal = t[sel, R.LT["NVALID"]] == 1           # p = 1: (1 - p) = 0, nothing to move
        p_one = np.exp(c["newlp"][i][sel].astype(np.float64)) == 1.0
        if sign == 0 or not passes:
            assert not moved.any(), (place, sign)
        else:
            assert moved[~one_legal & ~p_one].all(), (place, sign)
    if not big:
        return
    # the other axes, counted from the oracle's own terms and decisions
    vd, vb = t[:, R.LT["VDELTA"]], dec[:, 2]
    if c["clip_value"]:
        beyond = np.abs(vd) > R.CEPS
        counts = {"+eps": (vd == R.CEPS).sum(), "-eps": (vd == -R.CEPS).sum(), "tie": (vd == 0).sum(),
                  "inside": ((vd != 0) & (np.abs(vd) < R.CEPS)).sum(), "beyond, clipped larger": (beyond & (vb == 2)).sum(),
                  "beyond, clipped smaller": (beyond & (vb == 0)).sum(),
                  "beyond +": (vd > R.CEPS).sum(), "beyond -": (vd < -R.CEPS).sum()}
        assert min(counts.values()) >= R.MIN_PER_CATEGORY, counts
        assert (vb[np.abs(vd) <= R.CEPS] != 2).all() and (vb[beyond] != 1).all()
        # on the boundary itself with the clipped branch taken: only "<=" passes this gradient
        assert ((np.abs(vd) == R.CEPS) & (vb == 1)).sum() >= (R.MIN_PER_CATEGORY if c["n"] > 1000 else 8)
    else:
        assert (vb == 0).all() and (vd == 0).all()
    nvalid = t[:, R.LT["NVALID"]]
    if "ones" in R.SHAPE_CASES[k][3]:
        assert (nvalid == A).all()
    else:
        for kind in R.MASK_KINDS:
            assert (c["mask_kind"][i] == kind).sum() >= R.MIN_PER_CATEGORY, kind
        one = c["mask_kind"][i] == "one"
        assert (nvalid[one] == 1).all() and (t[one, R.LT["H"]] == 0).all() and (ratio[one & (pol < 2)] == 1).all()
        assert (c["newlp"][i][one] == 0).all() and (nvalid[c["mask_kind"][i] == "all"] == A).all()
        assert (nvalid[c["mask_kind"][i] == "two"] == 2).all()
        m, a = c["mask"][i].astype(bool), c["act"][i]
        assert (m.argmax(axis=1)[c["mask_kind"][i] == "first"] == a[c["mask_kind"][i] == "first"]).all()
        assert ((A - 1 - m[:, ::-1].argmax(axis=1))[c["mask_kind"][i] == "last"] == a[c["mask_kind"][i] == "last"]).all()
    for kind in R.LOGIT_KINDS:
        assert (c["logit_kind"][i] == kind).sum() >= R.MIN_PER_CATEGORY, kind


def test_std_zero_case_is_finite_and_normalizes_by_1e_minus_8():
    (k,) = [k for k, c in enumerate(R.SHAPE_CASES) if "std0" in c[3]]
    c = R.case_inputs(7, k)
    assert c["mb_stats"][1] == 0 and (np.abs(c["adv_n"][c["policy"] < 20]) > 0.25).all()
    assert np.array_equal(c["adv_n"], (c["adv"] - c["mb_stats"][0]) / F32(1e-8))


# ------------------------------------------------------------ (d) fragile cap --
@pytest.mark.parametrize("A,k", R.ALL_CASES)
def test_cases_stay_inside_the_fragile_cap(A, k):
    exact, sabs = R.case_reference(A, k)["metrics"]
    assert R.metric_fragile_count(exact, sabs, R.SHAPE_CASES[k][0]) <= R.metric_fragile_cap()


# ------------------------------------------- bppo_debug_wide_loss's argument checks --
def test_wide_loss_hook_checks_its_arguments():
    import bppo._lib as L
    c = R.case_inputs(7, 2)
    dout = np.zeros(c["n"] * 8 + R.GUARD, F32)
    met = np.zeros(R.WM_COUNT + 1 + R.GUARD, F32)
    p = lambda a: a.ctypes.data

    def call(A=7, n=c["n"], start=c["start"], perm=c["perm"], act=c["act"], buf_rows=c["buf_rows"], logp=p(c["logp"])):
        return L.lib().bppo_debug_wide_loss(A, n, start, perm.size, buf_rows, p(perm), p(act), logp, p(c["adv"]),
                                            p(c["ret"]), p(c["val"]), p(c["mask"]), p(c["logits_mb"]), p(c["values_mb"]),
                                            p(c["mb_stats"]), R.EPS, R.ENT_COEF, R.VALUE_COEF, 1, p(dout), p(met))
    for A in (0, 1, 3, 8, 32, 48, 50):
        assert call(A=A) == L.ERR_ARG, A
    assert call(n=0) == L.ERR_ARG and call(start=c["perm"].size) == L.ERR_ARG and call(logp=None) == L.ERR_ARG
    assert call(start=c["perm"].size - c["n"] + 1) == L.ERR_ARG              # start + n = perm_len + 1
    assert call(buf_rows=0) == L.ERR_ARG
    assert call(buf_rows=int(c["perm"].max())) == L.ERR_ARG                 # a perm entry == buf_rows
    bad = c["act"].copy()
    bad[3] = 7
    assert call(act=bad) == L.ERR_ARG


# -------------------------------------------- the pure-placement runs' preconditions --
@pytest.mark.parametrize("name", list(R.PURE_VARIANTS))
def test_pure_placements_craft_and_matter(name):
    """on the oracle alone: the search reaches every target for at least 90 % of a rollout's rows,
    the oracle's own ratio is then the target (its clip count says so: |hi - 1| and |lo_out - 1|
    exceed f32(0.2), |lo - 1| does not), and the placement matters: the policy head's gradient at
    exactly hi differs from the one a step above by more than 100 bars, likewise at lo"""
    import bppo
    from parity_util import oracle_train_cfg
    over, _ = R.PURE_VARIANTS[name]
    cfg = R.pure_config(over)
    params = bppo.orthogonal_init(cfg, seed=R.PURE_INIT_SEED)
    ot = O.Trainer(oracle_train_cfg(cfg), params)
    try:
        ot.collect(); ot.gae()
        B = R.PURE_N * R.PURE_T
        g = {}
        for place in R.PURE_PLACES:
            olp, found, go, ms = R.pure_reference(ot, cfg, params, place)
            assert found.mean() >= R.PURE_MIN_CRAFTED, (place, found.mean())
            count = R.pure_clip_count(ms)
            assert count == round(count)
            assert (count <= B - found.sum()) if place == "lo" else (count >= found.sum()), (place, count)
            g[place] = go
        tensors, total = R.pure_tensors(cfg)
        assert total == g["hi"].size
        (off, n) = tensors[-4]                                                 # the policy head's weights
        for a, b in (("hi", "hi_out"), ("lo", "lo_out")):
            d = np.abs(g[a][off:off + n] - g[b][off:off + n]).max()
            assert d > 100 * R.PURE_TOL * np.abs(g[a][off:off + n]).max(), (a, b, d)
    finally:
        ot.close()
