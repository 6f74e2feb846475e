"""The per-row PPO loss on the device, row by row and on its clip boundaries (tests/loss_rows_ref.py
holds the rule, the case tables and the seeds; tests/test_loss_rows_ref.py settles without a GPU
that the crafted rows land where intended and that the reference is the oracle's own row loop):

  k_wide_loss<A>, A in {2, 7, 33, 49}, through bppo_debug_wide_loss: every entry of dOut [n][A + 1]
  against or_loss_rows bit for bit, the metric slots against exact sums of the oracle's per-row
  terms (counts and the maximum exact; sums bit for bit unless fragile, then one ulp), a NaN prefill
  and guard bands behind both outputs;

  the CartPole kernels, which expose no rows, on PURE placements: every row of one minibatch at
  ratio exactly hi, exactly lo, one step above hi or one step below lo, so that a wrong routing
  of the boundary flips about half of the buffer's policy gradient: k_minibatch_mfma (mode 1),
  k_minibatch_split<true> (mode 0), k_minibatch<16,1,tanh>, k_minibatch<32,2,relu> and the GEMM
  path at hidden_size 48 (k_wide_loss<2>)."""
import ctypes as C

import numpy as np
import pytest

import bppo
import bppo._lib as L
import loss_rows_ref as R
import oracle_ffi as O
import update_kernels_ref as U
from parity_util import bits, oracle_train_cfg, summand_magnitude

pytestmark = pytest.mark.gpu
F32 = np.float32


# ============================================================== k_wide_loss ==
def _wide_loss(c):
    A, n = c["A"], c["n"]
    dout = np.full(n * (A + 1) + R.GUARD, np.nan, F32)
    met = np.full(R.WM_COUNT + 1 + R.GUARD, np.nan, F32)
    guard = np.arange(R.GUARD, dtype=F32) + F32(0.5)
    dout[n * (A + 1):] = guard
    met[R.WM_COUNT + 1:] = guard
    p = lambda a: a.ctypes.data
    st = L.lib().bppo_debug_wide_loss(A, n, c["start"], c["perm"].size, c["buf_rows"], p(c["perm"]), p(c["act"]),
                                      p(c["logp"]), p(c["adv"]), p(c["ret"]), p(c["val"]), p(c["mask"]),
                                      p(c["logits_mb"]), p(c["values_mb"]), p(c["mb_stats"]), R.EPS, R.ENT_COEF,
                                      R.VALUE_COEF, c["clip_value"], p(dout), p(met))
    assert st == L.OK, st
    assert np.array_equal(bits(dout[n * (A + 1):]), bits(guard)) and np.array_equal(bits(met[R.WM_COUNT + 1:]), bits(guard))
    return dout[:n * (A + 1)].reshape(n, A + 1), met[:R.WM_COUNT + 1]


def _describe(c, ref, r):
    b = c["idx"][r]
    return dict(row=int(r), policy=R.POLICY[c["policy"][b]], mask=str(c["mask_kind"][b]), logits=str(c["logit_kind"][b]),
                ratio=float(ref["terms"][r, R.LT["RATIO"]]), vdelta=float(ref["terms"][r, R.LT["VDELTA"]]),
                decisions=ref["dec"][r].tolist())


@pytest.mark.parametrize("A,k", R.ALL_CASES)
def test_wide_loss_rows(A, k):
    c, ref = R.case_inputs(A, k), R.case_reference(A, k)
    n = c["n"]
    dout, met = _wide_loss(c)
    assert not np.isnan(dout).any(), np.argwhere(np.isnan(dout))[:4]            # every row written
    bad = np.argwhere(bits(dout) != bits(ref["dout"]))
    assert bad.size == 0, (len(bad), [(int(a), float(dout[r, a]), float(ref["dout"][r, a]), _describe(c, ref, r))
                                      for r, a in bad[:4]])
    exact, sabs = ref["metrics"]
    for s in R.COUNT_SLOTS:
        assert met[R.WM[s]] == exact[R.WM[s]], (s, met[R.WM[s]], exact[R.WM[s]])
    vemax = F32(exact[R.WM["VEMAX"]])
    assert bits(met[R.WM["VEMAX"]]) == bits(vemax) == bits(met[R.VEMAX_LOCAL]), (met[R.WM["VEMAX"]], met[R.VEMAX_LOCAL], vemax)
    sums = [R.WM[s] for s in R.SUM_SLOTS]
    n_frag = U.check_outputs(met[sums], exact[sums], sabs[sums], n, (A, k, R.SUM_SLOTS))
    assert n_frag <= R.metric_fragile_cap(), n_frag



# ============================== the CartPole kernels on pure placements ==
@pytest.mark.parametrize("place", R.PURE_PLACES)
@pytest.mark.parametrize("name", list(R.PURE_VARIANTS))
def test_cartpole_kernels_on_pure_placements(name, place):
    from parity_util import cartpole_pair, cmp_cartpole_rollout
    over, mode = R.PURE_VARIANTS[name]
    cfg, tr, ot = cartpole_pair(R.PURE_N, R.PURE_T, num_epochs=1, num_minibatches=1, init_seed=R.PURE_INIT_SEED, **over)
    try:
        assert cfg == R.pure_config(over)
        if mode is not None:
            tr.ctx.set_minibatch_kernel(mode)
        bppo.collect_rollouts(tr.ctx); ot.collect()
        cmp_cartpole_rollout(tr, ot)                       # the stored log-probs are the oracle's, bit for bit
        tr.ctx.set_buffer("rewards", ot.buffer("rewards"))   # return normalizer: rtol 2e-7 (merge order)
        bppo.compute_gae(tr.ctx); ot.gae()
        assert np.array_equal(bits(tr.buffer.advantages.reshape(-1)), bits(ot.buffer("advantages")))
        p0 = tr.model.get_params()
        olp, found, go, ms = R.pure_reference(ot, cfg, p0, place)
        assert found.mean() >= R.PURE_MIN_CRAFTED, found.mean()
        tr.ctx.set_buffer("log_probs", olp)
        B = R.PURE_N * R.PURE_T
        lr, ent = bppo.schedule_get(cfg["learning_rate"], 0), bppo.schedule_get(cfg["entropy_coef"], 0)
        m = bppo.ppo_update(tr.ctx, lr, ent)
        rows = tr.ctx.minibatch_rows()
        assert len(rows) == 1 and rows[0][R.WM["N"]] == B
        # the clip count is exact: |ratio - 1| > f32(0.2) holds at hi, a step above it and a step
        # below lo, not at lo, so one row whose device ratio is a step off the target shows here
        count = R.pure_clip_count(ms)
        print(f"\n{name} at {place}: crafted {found.mean():.4f}, clip count {rows[0][R.WM['CF']]:.0f} (oracle {count:.0f})")
        assert rows[0][R.WM["CF"]] == count, (rows[0][R.WM["CF"]], count)
        floors = {"policy_loss": summand_magnitude(ot.buffer("advantages")), "value_loss": 0.0, "entropy": 0.0,
                  "approx_kl": 0.0, "clip_fraction": 1.0 / B}
        for k, fl in floors.items():
            o = getattr(ms, k)
            assert abs(m[k] - o) <= R.PURE_TOL * max(abs(o), fl), (k, m[k], o)
        g = tr.ctx.buffer("grad")
        tensors, total = R.pure_tensors(cfg)
        assert total == go.size == g.size
        for off, n in tensors:
            a, b = g[off:off + n], go[off:off + n]
            np.testing.assert_allclose(a, b, rtol=0, atol=R.PURE_TOL * max(np.abs(b).max(), 1e-30),
                                       err_msg=f"tensor at {off} ({n} entries), {name} at {place}")
    finally:
        tr.close(); ot.close()
