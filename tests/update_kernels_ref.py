"""Case tables, inputs and exact references for the update's small kernels (k_update.hip:
advantage statistics, slab reduction, clip + Adam), shared by tests/test_update_kernels_ref.py
(no GPU: fragility caps, the Adam restatement against the oracle) and
tests/test_gpu_update_kernels.py (the kernels through bppo_debug_adv_stats / _slab_reduce / _adam).

The rule for every exact comparison: the reference is exact arithmetic on the f32 inputs,
rounded once to f32.  Sums come from math.fsum over f64 terms that are exact (an f32, or a
product of two f32), so the f64 value handed to the rounding is the exact one rounded to f64
(relative error <= 2^-53; a mean's division adds another).  The device sums the same terms in
f64 in another order, which is off by at most L 2^-53 sum|terms| for L terms.  An output is
FRAGILE when rounding exact -+ L 2^-53 sum|terms| to f32 gives two different floats; only there
may the device differ from the reference, by one ulp.  The reference's own f64 roundings lie
inside that band whenever L >= 2 (and a one-term sum is exact), so where they could move the
f32 result the output is fragile and either neighbour is accepted."""
import functools
import math

import numpy as np

F32 = np.float32
U53 = 2.0 ** -53

# k_update.hip / bppo_internal.h constants the cases are built around
NUM_M, M_VEMAX = 11, 9                  # metric slots behind the parameters; the max slot
SLAB_GROUPS, SLAB_GUARD = 32, 64
ADAM_CHUNK, RED_SCRATCH_DOUBLES = 4096, 4 * 1024 + 64
GRAD_METRIC_SLOTS, GRAD_VEMAX, GRAD_VEMAX_LOCAL = 14, 9, 14
ADV_STREAM_BLOCKS, ADV_STREAM_MAXM = 512, 16


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def ulp32(x):
    x = F32(abs(x))
    return float(np.nextafter(x, F32(np.inf)) - x)


def ulps_apart(a, b):
    """distance in f32 steps between two finite floats (ordered-integer form)"""
    def key(v):
        u = int(np.array(v, F32).view(np.uint32))
        return u if u < 0x80000000 else 0x80000000 - u
    return abs(key(a) - key(b))


def fragile(exact, sum_abs, L):
    """exact: the exact value (as f64), sum_abs: sum |terms|, L: term count -> True when the f64
    summation error band around exact straddles an f32 rounding boundary"""
    band = L * U53 * sum_abs
    return F32(exact - band) != F32(exact + band)


def check_outputs(dev, exact, sum_abs, L, what):
    """dev [n] f32 against exact [n] f64 by the rule; -> the number of fragile outputs"""
    dev = np.asarray(dev, F32)
    n_frag = 0
    for i in range(dev.size):
        ref = F32(exact[i])
        if fragile(exact[i], sum_abs[i], L if np.isscalar(L) else L[i]):
            n_frag += 1
            assert ulps_apart(dev[i], ref) <= 1, (what, i, float(dev[i]), float(ref), "fragile, > 1 ulp")
        else:
            assert bits(dev[i]) == bits(ref), (what, i, float(dev[i]), float(ref), "not fragile, differs")
    return n_frag


def fragile_cap(n_outputs):
    return max(1, n_outputs // 1000)


# ====================================================== advantage statistics ==
def adv_plan(B, M, have_inv):
    """launch_epoch_adv_stats' plan: (path, C, nblk); path 0 = k_adv_epoch over the
    permutation, 4 / 8 / 16 = k_adv_stream<path> over its inverse"""
    base = B // M
    if have_inv and M <= ADV_STREAM_MAXM and base > 0:
        C = (B + ADV_STREAM_BLOCKS - 1) // ADV_STREAM_BLOCKS
        return (4 if M <= 4 else 8 if M <= 8 else 16), C, (B + C - 1) // C
    C = (B + 511) // 512
    if base > 0 and C > base:
        C = base
    if base == 0:
        C = 1
    return 0, C, (B + C - 1) // C


def mb_bounds(B, M):
    base, rem = B // M, B % M
    start = [m * base + min(m, rem) for m in range(M + 1)]
    return list(zip(start[:-1], start[1:]))


BIG = 2 ** 21 + 513        # C > 4096 in both kernels: a block runs more than one load round
# (B, M): every B meets a ragged M, every stream width an even and a ragged split; M > 16, B < M
# (base == 0, one row per block, empty minibatches), n = 1 minibatches; (1000, 24): M > 16 with
# blocks of 2 positions; the C = base cap of the permutation path needs ceil(B / 512) > B // M with at most
# 520 blocks: (65537, 512) takes it with C = base + 1; (51282, 518), base 99, with C = base + 2 =
# 101: uncapped, block 49 = [4949, 5050) would hold the last row of minibatch 49, all of 50 and
# the first row of 51, three minibatches for a kernel that keeps two slots
ADV_CASES = [
    (1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (5, 2), (5, 5), (5, 8),
    (511, 3), (511, 7), (511, 17), (512, 4), (512, 9), (512, 16), (512, 32),
    (513, 2), (513, 8), (513, 12), (1000, 3), (1000, 8), (1000, 12), (1000, 16), (1000, 17), (1000, 24),
    (4099, 1), (4099, 5), (4099, 16), (4099, 32), (65537, 4), (65537, 9), (65537, 512), (51282, 5), (51282, 518),
    (BIG, 3), (BIG, 5), (BIG, 16),
]
ADV_KINDS = ("n01", "mean10", "mean1000", "equal", "planted")
# At B = BIG a minibatch has n >= 2^17 rows.  For N(0,1) advantages the band n 2^-53 sum|a| / n
# = n 2^-53 0.8 is then 2^-36.3 .. 2^-33.9, while the mean, ~ n^-1/2 = 2^-8.5 .. 2^-9.7, has an f32
# step of 2^-32 .. 2^-34: the band is a tenth of the step at M = 16 and more than the whole step
# at M = 3, so most means are fragile under every seed and no seed meets the cap.  The zero-mean
# kind is therefore not run at BIG (it runs at every smaller B), and the planted vector there
# sits on N(10, 1) instead of N(0, 1): the f32 step of a mean near 10 is 2^-20, a dropped or
# double-counted planted row still moves the mean by >= 40 / n > 2^-15.
def adv_kinds(B):
    return ADV_KINDS if B < 2 ** 20 else ("mean10", "mean1000", "equal", "planted")


def planted_base(B):
    return F32(0.0) if B < 2 ** 20 else F32(10.0)
EQUAL_VALUE = F32(0.7310586)
# seeds under which every (case, kind) stays inside the fragile cap (settled on the CPU by
# tests/test_update_kernels_ref.py); a case not listed uses seed 0
ADV_SEEDS = {(512, 32, 'mean10'): 2, (65537, 512, 'n01'): 5, (65537, 512, 'mean1000'): 8}


def adv_seed(B, M, kind):
    return ADV_SEEDS.get((B, M, kind), 0)


def adv_inputs(B, M, kind, seed=None):
    """-> adv [B] f32, perm [B] u32 (shuffled position -> row), inv [B] u32 (row -> position)"""
    seed = adv_seed(B, M, kind) if seed is None else seed
    rng = np.random.default_rng([B, M, ADV_KINDS.index(kind), seed])
    perm = rng.permutation(B).astype(np.uint32)
    inv = np.empty(B, np.uint32)
    inv[perm] = np.arange(B, dtype=np.uint32)
    z = rng.standard_normal(B).astype(F32)
    if kind == "n01":
        adv = z
    elif kind == "mean10":
        adv = (z + F32(10.0)).astype(F32)
    elif kind == "mean1000":
        adv = (z + F32(1000.0)).astype(F32)
    elif kind == "equal":
        adv = np.full(B, EQUAL_VALUE, F32)
    else:
        # distinctive values on both sides of every chunk edge of both kernels (the stream
        # kernel chunks rows, the permutation kernel shuffled positions), then the extremes of
        # each minibatch on its first and last shuffled position: +-(1000 + m), so the global
        # extremes sit at the epoch's first and last minibatch edge and every minibatch's
        # min and max are its own
        adv = (z + planted_base(B)).astype(F32)
        _, Cs, _ = adv_plan(B, M, True)
        _, Cp, _ = adv_plan(B, M, False)
        for C, rows_of in ((Cs, None), (Cp, perm)):
            first = np.arange(0, B, C)
            last = np.minimum(first + C, B) - 1
            k = np.arange(first.size)
            fr, lr = (first, last) if rows_of is None else (rows_of[first], rows_of[last])
            adv[lr] = (-50.0 - (k % 5)).astype(F32)
            adv[fr] = (50.0 + (k % 7)).astype(F32)
        for m, (s, e) in enumerate(mb_bounds(B, M)):
            if e > s:
                adv[perm[e - 1]] = F32(-(1000.0 + m))
                adv[perm[s]] = F32(1000.0 + m)
    return np.ascontiguousarray(adv, F32), perm, inv


@functools.lru_cache(maxsize=8)
def adv_reference(B, M, kind, seed=None):
    """per minibatch: n, mean (exact, f64), sum|a| / n, min, max, std (the oracle's two-pass form
    in exact arithmetic: about the f32 mean, f32 variance, f32 sqrt), kappa = sum a^2 / sum (a - mean)^2"""
    adv, perm, _ = adv_inputs(B, M, kind, seed)
    return [rows_reference(adv[perm[s:e]]) for s, e in mb_bounds(B, M)]


def rows_reference(rows):
    """one minibatch's rows (f32) -> its entry of adv_reference"""
    n = len(rows)
    if n == 0:
        return dict(n=0)
    x = np.asarray(rows, F32).astype(np.float64)
    mean = math.fsum(x.tolist()) / n
    r = dict(n=n, mean=mean, mabs=float(np.abs(x).sum()) / n, min=F32(x.min()), max=F32(x.max()))
    if n > 1:
        d = x - float(F32(mean))
        v = math.fsum((d * d).tolist())
        r["std"] = np.sqrt(F32(v / (n - 1)))
        r["kappa"] = math.fsum((x * x).tolist()) / v if v > 0 else math.inf
    return r


def check_adv_stats(stats4, r, what):
    """device [mean, std, min, max] of one minibatch with >= 2 rows that are not all equal
    against its reference entry, by the bars of tests/test_gpu_update_kernels.py -> (the mean is
    fragile, std error / bound)"""
    mean, std, mn, mx = (F32(v) for v in stats4)
    assert bits(mn) == bits(r["min"]) and bits(mx) == bits(r["max"]), (what, mn, mx, r)
    frag = check_outputs([mean], [r["mean"]], [r["mabs"]], r["n"], (what, "mean"))
    tol = float(r["std"]) * 0.5 * r["kappa"] * r["n"] * U53 + 1.5 * ulp32(r["std"])
    err = abs(float(std) - float(r["std"]))
    assert err <= tol, (what, float(std), float(r["std"]), err, tol)
    return frag, err / tol


def adv_fragile_count(ref):
    return sum(1 for r in ref if r["n"] and fragile(r["mean"], r["mabs"], r["n"]))


# ============================================================ slab reduction ==
CFGB_PARAMS = 5 * 64 + 64 + 64 * 64 + 64 + 64 * 2 + 2 + 64 + 1
SLAB_ROWS = (1, 31, 32, 33, 255, 256, 1024)
SLAB_WIDTHS = (NUM_M + 1, 47, 48, 49, CFGB_PARAMS + NUM_M)
SLAB_CASES = [(r, w) for r in SLAB_ROWS for w in SLAB_WIDTHS]
SLAB_SEEDS = {}
SLAB_MAX = F32(7.5)


def slab_inputs(rows, width, max_row, seed=None):
    """entries of mixed magnitude and sign; the max column holds positive values below
    SLAB_MAX (so its sum and its max differ) and SLAB_MAX in row max_row"""
    seed = SLAB_SEEDS.get((rows, width), 0) if seed is None else seed
    rng = np.random.default_rng([rows, width, seed])
    slab = (rng.standard_normal((rows, width)) * 10.0 ** rng.uniform(-3, 3, (rows, width))).astype(F32)
    col = width - NUM_M + M_VEMAX
    slab[:, col] = rng.uniform(0.1, 5.0, rows).astype(F32)
    slab[max_row, col] = SLAB_MAX
    return slab


@functools.lru_cache(maxsize=4)
def slab_reference(rows, width, seed=None):
    """column sums (exact, f64) and sum |entries| of the sum columns; the planted row does not
    touch them"""
    slab = slab_inputs(rows, width, 0, seed).astype(np.float64)
    exact = np.array([math.fsum(c) for c in slab.T.tolist()])
    return exact, np.abs(slab).sum(axis=0)


def slab_fragile_count(rows, width, seed=None):
    exact, sabs = slab_reference(rows, width, seed)
    col = width - NUM_M + M_VEMAX
    return sum(1 for p in range(width) if p != col and fragile(exact[p], sabs[p], rows))


# =============================================================== clip + Adam ==
CFGB_TENSORS = (5 * 64, 64, 64 * 64, 64, 64 * 2, 2, 64, 1)     # w, b of hidden, hidden, policy, value
ADAM_TABLES = {
    "one": (1,), "chunk": (4096,), "chunk-1+1": (4095, 1), "chunk+1": (4097,), "two chunks+1": (8193, 64, 1),
    "cfgB": CFGB_TENSORS, "512x512": (512 * 512, 512),
}
MAX_NORM, ADAM_EPS, LR = F32(0.5), F32(1e-5), F32(1e-3)
# (step, gradient kind, world, from zero moments): the chain runs in this order, each step
# from the reference's previous state unless it starts fresh.  Kinds: "mixed<r>" gives tensor
# i the role (i + r) % 3 of far above max_norm / far below / all zero
ADAM_STEPS = [(1, "mixed0", 1, True), (1, "zero", 1, True), (1, "big", 1, True), (2, "small", 1, False),
              (1000, "big", 1, False), (3, "mixed1", 2, False), (4, "mixed2", 1, False), (5, "zero", 1, False)]
ADAM_SEEDS = {}


def powi_f32(a, b):
    a, r = F32(a), F32(1.0)
    while True:
        if b & 1:
            r = F32(r * a)
        b //= 2
        if b == 0:
            return r
        a = F32(a * a)


def adam_grad(lens, kind, seed):
    rng = np.random.default_rng([sum(lens), len(lens), seed])
    out = []
    for i, n in enumerate(lens):
        role = {"big": 0, "small": 1, "zero": 2}.get(kind)
        if role is None:
            role = (i + int(kind[-1])) % 3
        z = rng.standard_normal(n)
        if role == 0:
            g = z * 3.0 + (2.0 if n == 1 else 0.0)          # norm ~ 3 sqrt(n) >> 0.5
        elif role == 1:
            g = z * 1e-3 / math.sqrt(n)                       # norm ~ 1e-3
        else:
            g = np.zeros(n)
        out.append(g.astype(F32))
    return np.concatenate(out)


def adam_norms(lens, grad, world):
    """per tensor: the exact sum of squares of grad / world (f64), for the norm and its
    fragility"""
    g = (np.asarray(grad, F32) * (F32(1.0) / F32(world))).astype(np.float64)
    off, out = 0, []
    for n in lens:
        x = g[off:off + n]
        out.append(math.fsum((x * x).tolist()))
        off += n
    return out


def norm_fragile(ss, L):
    """the f32 norm sqrt(ss) under the f64 summation error of L positive terms, plus the
    square root's own f64 rounding"""
    lo = math.sqrt(ss * (1.0 - L * U53)) * (1.0 - 2 * U53)
    hi = math.sqrt(ss * (1.0 + L * U53)) * (1.0 + 2 * U53)
    return F32(lo) != F32(hi)


def adam_ref(lens, step, world, lr, max_norm, eps, grad, params, m1, m2):
    """or_adam_step (oracle/net.c) restated in numpy float32 operations over a table of
    back-to-back tensors, the gradient scaled by 1 / world first (k_adam's inv_world); every
    operation rounds to f32 once, as the C does.  -> params, m1, m2, clipped [nt]"""
    b1, b2 = F32(0.9), F32(0.999)
    f1, f2 = F32(F32(1.0) - b1), F32(F32(1.0) - b2)
    c1, c2 = F32(F32(1.0) - powi_f32(b1, step)), F32(F32(1.0) - powi_f32(b2, step))
    g = np.asarray(grad, F32) * F32(F32(1.0) / F32(world))
    p, m1, m2 = (np.array(a, F32) for a in (params, m1, m2))
    clipped = []
    for t, (ss, off) in enumerate(zip(adam_norms(lens, grad, world), np.cumsum((0,) + tuple(lens))[:-1])):
        sl = slice(off, off + lens[t])
        norm = F32(math.sqrt(ss))
        gt = g[sl]
        clipped.append(bool(norm > F32(max_norm)))
        if clipped[-1]:
            gt = gt * F32(F32(max_norm) / norm)
        m1[sl] = m1[sl] * b1 + gt * f1
        m2[sl] = m2[sl] * b2 + (gt * gt) * f2
        upd = (m1[sl] / c1) / (np.sqrt(m2[sl] / c2) + F32(eps))
        p[sl] = p[sl] - upd * F32(lr)
    assert g.dtype == p.dtype == m1.dtype == m2.dtype == F32
    return p, m1, m2, clipped


def adam_chain(name):
    """the table's steps: (step, world, grad, state before, reference state after, clipped)"""
    lens = ADAM_TABLES[name]
    n = sum(lens)
    rng = np.random.default_rng([n, 77])
    p0 = (rng.standard_normal(n) * 0.1).astype(F32)
    state = None
    out = []
    for k, (step, kind, world, fresh) in enumerate(ADAM_STEPS):
        if fresh or state is None:
            state = (p0.copy(), np.zeros(n, F32), np.zeros(n, F32))
        grad = adam_grad(lens, kind, ADAM_SEEDS.get((name, k), k))
        after = adam_ref(lens, step, world, LR, MAX_NORM, ADAM_EPS, grad, *state)
        out.append(dict(step=step, world=world, kind=kind, grad=grad, before=state, after=after[:3], clipped=after[3]))
        state = after[:3]
    return out


def threshold_cases():
    """four entries of 0.25 with max_norm 0.5: every square and every partial sum is exact in
    f64 in any order.  +0 ulp: the norm equals max_norm (not clipped).  +1 ulp in one entry:
    sqrt(0.25 (1 + 2^-24)) = 0.5 + 2^-26 rounds back to 0.5f, so the f32 norm still equals
    max_norm (not clipped, by the oracle's own comparison of the f32 norm).  +3 ulp: the norm is
    the next float above 0.5 (clipped)."""
    out = []
    for k, want in ((0, False), (1, False), (3, True)):
        g = np.full(4, 0.25, F32)
        for _ in range(k):
            g[2] = np.nextafter(g[2], F32(1.0))
        out.append((k, g, want))
    return out
