"""Case tables, crafted rows and references for the per-row PPO loss (ppo.rs:1385-1502 loss,
1507-1592 metrics), shared by tests/test_loss_rows_ref.py (no GPU: the oracle's row loop against
or_minibatch_loss_grad and against f64 autograd, the crafted rows' truth table, the fragile cap)
and tests/test_gpu_loss_rows.py (k_wide_loss<A> through bppo_debug_wide_loss, and the CartPole
minibatch kernels on pure ratio placements).

The reference of every row is or_loss_rows (oracle/net.c), the row loop of
or_minibatch_loss_grad.  Its three decisions, and the lines they restate:

    rhs     = pl1 < pl2                 ppo.rs:1452-1458 max_pair(-A r, -A clamp(r)): a tie takes
                                        the first (unclipped) operand
    g_ratio = (!rhs || lo <= r <= hi)   Burn's clamp passes the gradient on its boundaries, so a
              ? -A_n / mb : 0           ratio exactly lo or hi is NOT cut
    value:    l1 < l2 ? clipped branch, gradient only if -eps <= v - v_old <= eps : unclipped
                                        ppo.rs:1467-1474, the same max_pair and clamp

Rows are built along four axes (policy placement x sign of A_n, value placement, mask, logits),
one category of each per row.  The policy axis is cyclic in the buffer row, the others are drawn
per row.  A case with n >= 1000 rows holds at least MIN_PER_CATEGORY rows of every category (the
CPU test counts them from the oracle's own decisions); the smaller shapes of the table (n = 1 ..
257, fewer rows than 16 x 21 policy categories) are windows of the same mixture.

Metric sums follow update_kernels_ref's rule: exact sums (math.fsum) of the oracle's f32 per-row
terms, rounded once; the device may differ by one ulp where the output is fragile, at most
fragile_cap(outputs) outputs per case.  dout is compared bit for bit: both sides form each entry
in f64 from the same f32 values with the same operations and round once."""
import ctypes as C
import functools
import math

import numpy as np

import oracle_ffi as O
import update_kernels_ref as U
from test_gpu_clip_value import craft_old_values

F32 = np.float32
EPS, ENT_COEF, VALUE_COEF = 0.2, 0.01, 0.5
CEPS = F32(EPS)
LO, HI = F32(1.0 - EPS), F32(1.0 + EPS)
ACTION_COUNTS = (2, 7, 33, 49)
GUARD = 64                                   # floats behind dout and behind the metric slots
# bppo_metric_row.h
WM = dict(PL=0, VL=1, H=2, KL=3, CF=4, V=5, R=6, VE=7, VE2=8, VEMAX=9, N=10, VALID=11, HV=12, NCHOICE=13)
WM_COUNT, VEMAX_LOCAL = 14, 14
# oracle.h
LT = dict(PL=0, VL=1, H=2, KL=3, CF=4, VE=5, NVALID=6, HV=7, RATIO=8, VDELTA=9)
LT_COUNT = 10
MIN_PER_CATEGORY = 16

# ------------------------------------------------------------------ policy axis --
PLACES = ("one", "hi", "lo", "hi_in", "hi_out", "lo_in", "lo_out", "far_hi", "far_lo", "inside")
EXACT_PLACES = ("hi", "lo", "hi_in", "hi_out", "lo_in", "lo_out")
POLICY = [(p, s) for p in PLACES for s in (+1, -1)] + [("inside", 0)]      # sign 0: A_n = +0
TARGET = {"hi": HI, "lo": LO, "hi_in": np.nextafter(HI, F32(0)), "hi_out": np.nextafter(HI, F32(2)),
          "lo_in": np.nextafter(LO, F32(2)), "lo_out": np.nextafter(LO, F32(0))}
# (placement, sign of A_n) -> (take_rhs, lo <= ratio <= hi, gradient passes).  With A_n > 0 the
# surrogate -A_n r falls with r, so the clipped operand is the larger one only above hi; with
# A_n < 0 only below lo.  On lo and hi themselves clamp(r) == r: a tie, unclipped, passes.
TRUTH = {}
for _p in PLACES:
    _in = _p in ("one", "hi", "lo", "hi_in", "lo_in", "inside")
    for _s in (+1, -1):
        _rhs = (_p in ("hi_out", "far_hi")) if _s > 0 else (_p in ("lo_out", "far_lo"))
        TRUTH[(_p, _s)] = (int(_rhs), int(_in), int(not _rhs or _in))
TRUTH[("inside", 0)] = (0, 1, 1)
assert {k for k, v in TRUTH.items() if not v[2]} == {("hi_out", 1), ("far_hi", 1), ("lo_out", -1), ("far_lo", -1)}

VALUE_KINDS = 8          # craft_old_values: 0 / 1 exactly +-eps, 2 / 3 beyond, 4 inside, 5..7 the tie
MASK_KINDS = ("one", "two", "all", "first", "last")
LOGIT_KINDS = ("std", "equal", "spread30", "dom100", "edge87")

# ------------------------------------------------------------------- case table --
GRID_N = 1024 * 256 + 300          # blocks is capped at 1024: the grid-stride loop's second round
# (n, start, clip_value, flags); flags: "ones" = all-ones masks (A = 2, the GEMM path of CartPole),
# "std0" = mb_stats std 0 (the denominator is 1e-8f), "grid" = only for A in GRID_ACTIONS
SHAPE_CASES = [
    (1, 0, 1, ""), (1, 5, 0, ""), (63, 0, 1, ""), (64, 3, 0, ""), (65, 0, 1, ""), (255, 7, 0, ""), (256, 0, 1, ""),
    (257, 2, 1, "std0"), (1000, 0, 1, ""), (1000, 11, 0, ""), (1000, 4, 1, "ones"), (GRID_N, 9, 1, "grid"),
]
GRID_ACTIONS = (2, 7)
EXTRA_ROWS, PERM_TAIL = 91, 5      # the buffer holds n + 91 rows, the permutation start + n + 5 entries


def cases(A):
    out = []
    for k, (n, start, cv, flags) in enumerate(SHAPE_CASES):
        if ("ones" in flags and A != 2) or ("grid" in flags and A not in GRID_ACTIONS):
            continue
        out.append(k)
    return out


ALL_CASES = [(A, k) for A in ACTION_COUNTS for k in cases(A)]
# seeds under which a case stays inside the fragile cap (tests/test_loss_rows_ref.py); default 0
SEEDS = {}
# or_loss_rows' dlogits / dv against f64 autograd, interior rows (more than 8 ulp from lo, hi and
# +-eps, no v == v_old tie), mb = 1 scaling: the worst row of every case per A as measured by
# tests/test_loss_rows_ref.py (it prints them), and the bar at 4x.  The quantity is the oracle's own
# f32 rounding, not the device's.  The worst rows are the dom100 ones whose taken log-prob is
# near -100: half an f32 step there, 2^-18 = 3.8e-6, is that much of the ratio.
# The denominator is the row's largest |gradient entry|, but not less than the magnitudes its
# entries are differences of: |A_n| ratio where the policy gradient passes (onehot - p with p
# rounded to f32 near 1) and ent_coef max_a p_a max(|ls_a|, H) (ls_a + H).  Measured against the
# largest entry alone, a row with equal logits and both gradients cut, whose exact gradient is 0,
# shows the f32 residue of ls_a + H (5e-10 of nothing), and a far_hi row with p = 1 - 4e-10
# shows e^10 A_n 4e-10 against a value gradient of 0.1: 3e-5, and up to 1e-2 under another seed.
# Measured with these tables (A: interior rows, share below the floors and left out, and for the plain
# measure the issue names -- error / the row's largest |entry|, rows with a nonzero gradient -- the
# median, the share of rows above the bar 1.6e-5, the worst row whose largest entry is >= 1e-3):
#    2: 43338 rows, 8.5 % left out; plain median 4.7e-8, 13.4 % above, worst 1.0
#    7: 43170 rows, 8.0 % left out; plain median 5.2e-8, 13.4 % above, worst 1.0
#   33:   821 rows, 2.7 % left out; plain median 3.4e-8,  4.3 % above, worst 3.8e-6
#   49:   826 rows, 1.9 % left out; plain median 3.5e-8,  2.8 % above, worst 1.8e-3
# The plain worst of 1.0 is a far_hi row, two legal actions 22 apart, p = 1 in f32: the oracle's
# entry of the taken action is e^10 A_n (1 - 1.0f) = 0 where f64 has 1.4e-3, the other entry
# (-p_other) agrees to 1e-6.  Burn's f32 autodiff forms onehot - softmax the same way.
AUTOGRAD_WORST = {2: 3.876e-06, 7: 3.966e-06, 33: 3.795e-06, 49: 3.856e-06}
AUTOGRAD_BAR = {A: 4 * w for A, w in AUTOGRAD_WORST.items()}
INTERIOR_ULPS = 8


# ------------------------------------------------------------------- host libm --
def _libm(which, x):
    """the host build of the library's restated glibc expf (4) / logf (0): no GPU"""
    import bppo._lib as L
    x = np.ascontiguousarray(x, F32)
    y = np.empty_like(x)
    assert L.lib().bppo_debug_libm(which, 0, x.ctypes.data, y.ctypes.data, x.size) == 0
    return y


def expf(x):
    x = np.asarray(x, F32)
    return _libm(4, x.ravel()).reshape(x.shape)


def logf(x):
    x = np.asarray(x, F32)
    return _libm(0, x.ravel()).reshape(x.shape)


def log_softmax_rows(x):
    """or_log_softmax_row over rows of x [n][A] f32: max, an f32 sum of expf in column order, logf"""
    x = np.asarray(x, F32)
    d = x - x.max(axis=1, keepdims=True)
    e = expf(d)
    s = np.zeros(x.shape[0], F32)
    for a in range(x.shape[1]):
        s = s + e[:, a]
    out = d - logf(s)[:, None]
    assert out.dtype == F32
    return out


def craft_old_logp(newlp, target):
    """old log-probs with expf(f32(newlp - olp)) == target bit for bit, searched among the f32
    neighbours of newlp - log(target) -> olp, found"""
    newlp = np.asarray(newlp, F32)
    base = (newlp.astype(np.float64) - math.log(float(target))).astype(F32)
    bi = base.view(np.int32)
    olp, found = base.copy(), np.zeros(newlp.size, bool)
    for k in sorted(range(-48, 49), key=abs):
        cand = (bi + np.int32(k)).view(F32)
        hit = (expf(newlp - cand) == target) & ~found
        olp[hit] = cand[hit]
        found |= hit
        if found.all():
            break
    return olp, found


def craft_boundary_off_value(v, d):
    """old values with f32(v - v_old) == d bit for bit and f32(v_old + d) != v -> v_old, found"""
    v = np.asarray(v, F32)
    bi = (v - d).view(np.int32)
    out, found = (v - d).astype(F32), np.zeros(v.size, bool)
    for k in sorted(range(-16, 17), key=abs):
        cand = (bi + np.int32(k)).view(F32)
        hit = ((v - cand) == d) & ((cand + d) != v) & ~found
        out[hit] = cand[hit]
        found |= hit
    return out, found


# ----------------------------------------------------------------- buffer rows --
def _masks_actions(rng, A, B, kind, ones):
    act = rng.integers(0, A, B).astype(np.int32)
    if ones:
        return np.ones((B, A), np.uint8), act
    rows = np.arange(B)
    mask = np.zeros((B, A), bool)
    mask[rows, act] = True
    k = np.array([MASK_KINDS.index(x) for x in kind])
    two = k == 1
    other = (act + 1 + rng.integers(0, A - 1, B)) % A
    mask[rows[two], other[two]] = True
    mask[k == 2] = True
    fl = k >= 3                                   # a random mask of at least min(3, A) legal actions
    r = rng.random((B, A))
    m = r < 0.6
    np.put_along_axis(m, np.argsort(r, axis=1)[:, :min(3, A)], True, axis=1)
    first = m.argmax(axis=1)
    last = A - 1 - m[:, ::-1].argmax(axis=1)
    mask[fl] = m[fl]
    act = np.where(k == 3, first, np.where(k == 4, last, act)).astype(np.int32)
    assert mask[rows, act].all()
    return mask.astype(np.uint8), act


def _logits(rng, A, B, kind, mask, act):
    rows = np.arange(B)
    k = np.array([LOGIT_KINDS.index(x) for x in kind])
    legal = mask.astype(bool)
    z = rng.standard_normal((B, A)).astype(F32)
    lg = z.copy()
    others = legal.copy()
    others[rows, act] = False
    has_other = others.any(axis=1)
    # "top": the column that dominates (dom100) or stays at 0 (edge87): the taken action, or for
    # half of the rows that have one, another legal action (the taken one is then the improbable)
    top = np.where((rng.random(B) < 0.5) & has_other, others.argmax(axis=1), act)
    eq = k == 1
    lg[eq] = rng.standard_normal(B).astype(F32)[eq, None]
    sp = k == 2
    lg[sp] = rng.uniform(-30.0, 30.0, (B, A)).astype(F32)[sp]
    dm = k == 3
    zl = np.where(legal, z, F32(-np.inf)).max(axis=1)
    lg[rows[dm], top[dm]] = (zl + F32(100.0))[dm]
    ed = k == 4
    lg[ed] = (z * F32(0.1) - rng.uniform(86.0, 89.0, (B, A)).astype(F32))[ed]
    lg[rows[ed], top[ed]] = (z[rows, top] * F32(0.1))[ed]
    # std: the taken action's probability among the legal ones is p in [0.5, 0.7]
    st = (k == 0) & has_other
    zo = np.where(others, z.astype(np.float64), -np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):      # rows without another legal action: unused
        lse = np.log(np.exp(zo - zo.max(axis=1, keepdims=True)).sum(axis=1)) + zo.max(axis=1)
    p = rng.uniform(0.5, 0.7, B)
    lg[rows[st], act[st]] = (lse + np.log(p / (1.0 - p))).astype(F32)[st]
    return np.ascontiguousarray(lg, F32)


@functools.lru_cache(maxsize=2)
def buffer_rows(A, B, seed, ones, std0, clip_seed=0):
    """B buffer rows -> dict: the kernel's buffer-indexed inputs, the rows' own logits and values,
    and what each row was meant to be (policy index into POLICY, crafted = the search succeeded)"""
    rng = np.random.default_rng([A, B, seed, int(ones), int(std0)])
    pol = np.arange(B) % len(POLICY)
    place = np.array([POLICY[i][0] for i in pol])
    sign = np.array([POLICY[i][1] for i in pol])
    mkind = np.array(MASK_KINDS)[rng.integers(0, len(MASK_KINDS), B)]
    lkind = np.array(LOGIT_KINDS)[rng.integers(0, len(LOGIT_KINDS), B)]
    exact = np.isin(place, EXACT_PLACES)
    lkind[exact] = "std"
    mask, act = _masks_actions(rng, A, B, mkind, ones)
    logits = _logits(rng, A, B, lkind, mask, act)
    x = logits + (mask.astype(F32) - F32(1.0)) * F32(1e9)
    newlp = log_softmax_rows(x)[np.arange(B), act]
    olp = newlp.copy()                                              # "one"
    crafted = np.ones(B, bool)
    for name, t in TARGET.items():
        sel = place == name
        olp[sel], crafted[sel] = craft_old_logp(newlp[sel], t)
    olp[place == "far_hi"] = (newlp - F32(10.0))[place == "far_hi"]
    olp[place == "far_lo"] = (newlp + F32(10.0))[place == "far_lo"]
    ins = place == "inside"
    olp[ins] = (newlp - rng.uniform(-0.15, 0.15, B).astype(F32))[ins]
    # advantages: A_n = (adv - mean) / (std + 1e-8f) of magnitude 0.3 .. 2; on the exact
    # placements 1.02 .. 1.18: one f32 step of the ratio (mantissa 1.2 at hi, 1.6 at lo) then
    # moves the product -A_n r by at least one step of ITS OWN (mantissa below 2), so pl1 and pl2
    # of a one-step-outside row cannot round to a tie
    mean, std = (F32(0.0), F32(0.0)) if std0 else (F32(0.25), F32(1.5))
    denom = F32(std + F32(1e-8))
    mag = np.where(exact, rng.uniform(1.02, 1.18, B), rng.uniform(0.3, 2.0, B))
    adv = (mean + (sign * mag * float(denom)).astype(F32)).astype(F32)
    adv[sign == 0] = mean
    adv_n = ((adv - mean) / denom).astype(F32)
    assert adv.dtype == F32 and (np.sign(adv_n) == sign).all() and np.isfinite(adv_n).all()
    # values N(0.5, 1), not N(0, 1): a sum of n zero-mean terms is ~ sqrt(n) with an f32 step far
    # below the f64 reordering band of its n terms, i.e. fragile under most seeds at the grid-stride
    # size (update_kernels_ref.py meets the same with its advantage means)
    # (the forward's value of the row; a quarter of them small, where the boundary search below succeeds)
    zv = rng.standard_normal(B)
    val = np.where(rng.random(B) < 0.25, 0.06 * zv, 0.5 + zv).astype(F32)
    old_val, _ = craft_old_values(val, CEPS, seed=clip_seed + seed)
    ret = (val + rng.normal(0.0, 0.5, B).astype(F32)).astype(F32)
    # a row exactly on +-eps as craft_old_values makes it has v_old = v -+ eps exactly, so
    # v_clipped = f32(v_old +- eps) == v: a tie of l1 and l2 whatever the kernel does with the
    # boundary.  Every other tie row (v_old == v) therefore looks for a v_old that keeps
    # f32(v - v_old) == +-eps by rounding, with v_clipped off v (found for small |v| only), and R
    # goes to the side that makes the clipped error the larger: the clipped branch is taken
    # and its gradient is passed only by a comparison that includes the boundary
    tie = np.flatnonzero(val == old_val)[::2]
    for d, sel in ((CEPS, tie[::2]), (-CEPS, tie[1::2])):
        alt, found = craft_boundary_off_value(val[sel], d)
        old_val[sel[found]] = alt[found]
    dlt = val - old_val
    vc = old_val + np.clip(dlt, -CEPS, CEPS)
    edge = (np.abs(dlt) == CEPS) & (vc != val)
    ret[edge] = (val - np.sign(vc - val) * np.abs(ret - val))[edge]
    assert ret.dtype == F32 and vc.dtype == F32
    return dict(A=A, B=B, act=act, logp=olp.astype(F32), adv=adv, adv_n=adv_n, ret=ret, val=old_val, mask=mask,
                logits=logits, values=val, mb_stats=np.array([mean, std], F32), policy=pol, crafted=crafted,
                mask_kind=mkind, logit_kind=lkind, newlp=newlp)


def case_inputs(A, k):
    """case k of SHAPE_CASES at A actions -> dict: the hook's arguments (buffer-indexed arrays of
    buf_rows rows, perm, start, n, minibatch-indexed logits / values) and idx = the minibatch's
    buffer rows"""
    n, start, cv, flags = SHAPE_CASES[k]
    B = n + EXTRA_ROWS
    seed = SEEDS.get((A, k), 0)
    b = buffer_rows(A, B, seed, "ones" in flags, "std0" in flags)
    rng = np.random.default_rng([A, k, seed, 1])
    perm = rng.permutation(B).astype(np.uint32)[:start + n + PERM_TAIL]
    idx = perm[start:start + n].astype(np.int64)
    assert not np.array_equal(idx, np.arange(n))
    return dict(b, n=n, start=start, clip_value=cv, perm=perm, idx=idx, buf_rows=B,
                logits_mb=np.ascontiguousarray(b["logits"][idx]), values_mb=np.ascontiguousarray(b["values"][idx]))


def oracle_rows(A, n, logits, values, act, logp, adv_n, ret, old_val, mask, clip_value, eps=EPS, ent=ENT_COEF,
                value_coef=VALUE_COEF):
    """or_loss_rows on minibatch-ordered rows -> dlogits [n][A], dv [n], terms [n][LT_COUNT], decisions [n][3]"""
    pc = O.ppo_cfg(clip=eps, value_coef=value_coef, clip_value=bool(clip_value))
    dl, dv = np.zeros((n, A), F32), np.zeros(n, F32)
    terms, dec = np.zeros((n, LT_COUNT), F32), np.zeros((n, 3), np.int32)
    mk = None if mask is None else np.ascontiguousarray(mask, F32)
    c = lambda a, t=F32: np.ascontiguousarray(a, t)
    O.lib().or_loss_rows(A, n, c(logits), c(values), c(act, np.int32), c(logp), c(adv_n), c(ret), c(old_val),
                         None if mk is None else mk.ctypes.data, C.byref(pc), ent, dl, dv, terms, dec)
    return dl, dv, terms, dec


@functools.lru_cache(maxsize=2)
def case_reference(A, k):
    """the oracle's rows of a case and the exact metric sums -> dict"""
    c = case_inputs(A, k)
    i = c["idx"]
    dl, dv, terms, dec = oracle_rows(A, c["n"], c["logits_mb"], c["values_mb"], c["act"][i], c["logp"][i],
                                     c["adv_n"][i], c["ret"][i], c["val"][i], c["mask"][i], c["clip_value"])
    return dict(dout=np.concatenate([dl, dv[:, None]], axis=1), terms=terms, dec=dec,
                metrics=metric_reference(terms, c["values_mb"], c["ret"][i]))


SUM_SLOTS = ("PL", "VL", "H", "KL", "V", "R", "VE", "VE2", "HV")
COUNT_SLOTS = ("CF", "N", "VALID", "NCHOICE")


def metric_reference(terms, values, ret):
    """-> exact [WM_COUNT] f64 (sums by math.fsum of exact f64 terms, counts, the max), sum |terms|"""
    t = terms.astype(np.float64)
    ve = t[:, LT["VE"]]
    choice = t[:, LT["NVALID"]] > 1.0
    cols = dict(PL=t[:, LT["PL"]], VL=t[:, LT["VL"]], H=t[:, LT["H"]], KL=t[:, LT["KL"]],
                V=np.asarray(values, np.float64), R=np.asarray(ret, np.float64), VE=ve, VE2=ve * ve,
                HV=t[choice, LT["HV"]])
    exact, sabs = np.zeros(WM_COUNT), np.zeros(WM_COUNT)
    for name, col in cols.items():
        exact[WM[name]] = math.fsum(col.tolist())
        sabs[WM[name]] = float(np.abs(col).sum())
    exact[WM["CF"]] = t[:, LT["CF"]].sum()
    exact[WM["N"]] = len(t)
    exact[WM["VALID"]] = t[:, LT["NVALID"]].sum()
    exact[WM["NCHOICE"]] = choice.sum()
    exact[WM["VEMAX"]] = ve.max()
    return exact, sabs


def metric_fragile_count(exact, sabs, n):
    return sum(1 for s in SUM_SLOTS if U.fragile(exact[WM[s]], sabs[WM[s]], n))


def metric_fragile_cap():
    return U.fragile_cap(len(SUM_SLOTS))


def interior(terms, clip_value):
    """rows whose f32 ratio is more than INTERIOR_ULPS steps from lo and hi and whose v - v_old is
    more than that from +-eps and not 0 (the tie)"""
    r, d = terms[:, LT["RATIO"]], terms[:, LT["VDELTA"]]
    far = lambda x, t: np.abs(x.view(np.int32).astype(np.int64) - int(np.array(t, F32).view(np.int32))) > INTERIOR_ULPS
    ok = far(r, LO) & far(r, HI)
    if clip_value:
        ok &= far(d, CEPS) & far(d, -CEPS) & (d != 0)
    return ok


# ============================================ the CartPole kernels on pure placements ==
# k_minibatch<H,NL,ACT>, k_minibatch_mfma and k_minibatch_split<exact_fwd> expose no rows, so a
# run puts EVERY row of one minibatch (N x T = 256 x 32, one epoch) on one placement: the old
# log-probs are rewritten so that the ratio of the update's first minibatch, whose forward
# reproduces the stored log-prob bit for bit, is exactly the target.  Advantages keep their mixed
# signs, so a kernel that routes the boundary wrongly cuts (or passes) about half of the rows.
PURE_N, PURE_T = 256, 32
PURE_PLACES = ("hi", "lo", "hi_out", "lo_out")
# name -> (config overrides, bppo_set_minibatch_kernel mode or None)
PURE_VARIANTS = {
    "k_minibatch_mfma": (dict(), 1),
    "k_minibatch_split<true>": (dict(), 0),
    "k_minibatch<16,1,tanh>": (dict(hidden_size=16, num_hidden=1, activation="tanh"), None),
    "k_minibatch<32,2,relu>": (dict(hidden_size=32, num_hidden=2, activation="relu"), None),
    "k_wide_loss<2> (hidden_size 48)": (dict(hidden_size=48), None),
}
PURE_TOL = 1e-5                 # of a gradient tensor's largest |entry|, and of the metrics
PURE_MIN_CRAFTED = 0.9
PURE_INIT_SEED = 3


def pure_config(over):
    import bppo
    cfg = bppo.make_config("cartpole", num_envs=PURE_N, num_steps=PURE_T, seed=42, num_epochs=1, num_minibatches=1,
                           **over)
    assert cfg["clip_epsilon"] == EPS and not cfg.get("clip_value")
    return cfg


def pure_tensors(cfg):
    """(offset, length) of every parameter tensor in record order: hidden layers, policy, value"""
    H, NL = cfg["hidden_size"], cfg["num_hidden"]
    shapes = [(5, H)] + [(H, H)] * (NL - 1) + [(H, 2), (H, 1)]
    out, off = [], 0
    for i, o in shapes:
        for n in (i * o, o):
            out.append((off, n))
            off += n
    return out, off


def pure_reference(ot, cfg, params, place):
    """the oracle trainer's collected and bootstrapped rollout with every old log-prob moved to
    `place` -> old log-probs, found, or_minibatch_loss_grad's gradient and statistics from params"""
    import bppo
    B = PURE_N * PURE_T
    olp, found = craft_old_logp(ot.buffer("log_probs"), TARGET[place])
    adv = ot.buffer("advantages")
    advn = np.zeros(B, F32)
    st = [C.c_float() for _ in range(4)]
    O.lib().or_normalize_advantages(adv, B, advn, *[C.byref(x) for x in st])
    desc = O.mlp_desc(5, 2, cfg["hidden_size"], cfg["num_hidden"], cfg["activation"] == "relu")
    pc = O.ppo_cfg(num_epochs=1, num_minibatches=1, clip=cfg["clip_epsilon"], value_coef=cfg["value_coef"])
    go, ms = np.zeros(desc.n_params, F32), O.MbStats()
    O.lib().or_minibatch_loss_grad(C.byref(desc), np.ascontiguousarray(params, F32), B, ot.buffer("obs"), None,
                                   ot.buffer("actions", np.int32), olp, advn, ot.buffer("returns"), ot.buffer("values"),
                                   None, C.byref(pc), bppo.schedule_get(cfg["entropy_coef"], 0), go, C.byref(ms))
    return olp, found, go, ms


def pure_clip_count(ms):
    return ms.clip_fraction * (PURE_N * PURE_T)          # k / 8192 is exact in f32
