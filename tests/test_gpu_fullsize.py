"""The benched paths at the sizes they run, against full-size oracle fixtures
(VERDICT r2, next-round item 1).

Each case runs ONE iteration of the exact bench path -- bppo_train_steps
(Trainer.train_updates): the fused packed update rows written by the rollout and
GAE, the speculative shuffle engine and the side-stream Fisher-Yates, the
pipelined host loop -- with no injected state, and compares it with the oracle
run of the same config that tests/golden/make_fullsize_fixtures.py recorded in
the build container (the oracle needs minutes to hours at these sizes):

  CfgB  CartPole N=65,536 T=128, 4 x 4 minibatches of 2,097,152 rows (bench.py)
  CfgC  Connect Four N=16,384 T=64, 6 x 4, target_kl 0.02 (scripts/bench_wide.py)
  CfgD  Liar's Dice CTDE N=32,768 T=128, 4 x 8, target_kl 0.025 (scripts/bench_wide.py)

Tolerances are those of tests/parity_util.py: bit-exact buffers by sha256 (the
CartPole rewards after the return normalizer's f64 block scan at rtol 2e-7 and the
advantages/returns downstream of them at 1e-5, on a fixed strided sample and
every step row's sum); metrics within 1e-5 relative (clip_fraction, a count: 4 rows
per minibatch); parameters rtol 1e-4 / atol 2e-5 for >= 99.9 % of a fixed sample and
within 1 % of lr per Adam step for all of it, per-tensor sums of |p - p0| within 1e-4
relative.

test_updates_without_injection_action_agreement runs K updates on both
sides with nothing injected between them and reports how long the trajectories
stay action-identical.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import bppo
import oracle_ffi as O
from parity_util import METRICS, PARAM_ATOL, PARAM_RTOL, RTOL, _floor, oracle_train_cfg, summand_magnitude

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
CASES = {   # = make_fullsize_fixtures.CASES (the fixture records its own copy, checked below)
    "cfgB": dict(preset="cartpole", num_envs=65536, num_steps=128, init_seed=1),
    "cfgC": dict(preset="connect_four", num_envs=16384, num_steps=64, init_seed=5),
    "cfgD": dict(preset="liars_dice_ctde", num_envs=32768, num_steps=128, init_seed=5),
}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint8)).hexdigest()


def _exact_buffers(cfg):
    out = [("actions", np.int32), ("dones", np.float32), ("obs", np.float32), ("values", np.float32),
           ("log_probs", np.float32)]
    if cfg["env"] != "cartpole":
        out += [("players", np.int32), ("masks", np.float32), ("rewards", np.float32),
                ("all_rewards", np.float32), ("advantages", np.float32), ("returns", np.float32)]
        if cfg["network_type"] == "ctde":
            out.append(("priv", np.float32))
    return out


def _layer_sizes(cfg):
    shapes, _ = bppo.host.layer_shapes(cfg)
    return [sz for i, n in shapes for sz in (i * n, n)]


def _check_minibatch_rows(rows, fx, mb, pl_mag, first_epoch_rows):
    """the minibatches of the update's first epoch (bppo_minibatch_rows) against the oracle's
    statistics of the same minibatch (or_trainer_mb_log, recorded in the fixture) at 1e-5;
    later epochs are reported, not asserted: the two trajectories' parameters differ in the
    last bits after the first Adam steps (Adam's m/sqrt(v) turns last-bit gradient differences
    of near-zero entries into steps of up to ~lr), which the KL of a policy that has moved
    amplifies (CfgC: approx_kl 2-7x the bar from minibatch 8 of 24, profiles/r06e/), and
    test_bench_minibatches_from_device_parameters holds EVERY minibatch at 1e-5 from the
    device's own parameters.  At the benched
    minibatch sizes and with the benched arithmetic: CfgB k_minibatch_split<true> (exact f32
    forward, split-bf16 backward) on the first minibatch and k_minibatch_split after; CfgC / CfgD the exact forward with f32 split-K
    weight gradients and the split-bf16 backward on the first minibatch, the split-bf16 GEMMs
    on the rest (>= 32,768 rows).  Each minibatch runs from the device's own parameters after
    its earlier Adam steps (ppo.rs:1923-1988).  Floors as for the update's metrics: the
    policy loss's summand magnitude, value/returns means their own magnitude; approx_kl an
    absolute 2^-24/sqrt(mb) (each row's (ratio-1) - log ratio from a ratio within f32
    resolution of 1); clip_fraction 4 rows of the minibatch (ratios within rounding of
    1 +- eps)."""
    fields = [str(f) for f in fx["mb_fields"]]
    log = [dict(zip(fields, (float(v) for v in r))) for r in fx["mb_log"]]
    assert len(rows) == len(log), (len(rows), len(log))
    worst, bad = [], []
    for k, (r, o) in enumerate(zip(rows, log)):
        n = float(r[10])
        assert n == mb, (k, n, mb)
        dev = {"policy_loss": r[0] / n, "value_loss": 0.5 * r[1] / n, "entropy": r[2] / n,
               "approx_kl": r[3] / n, "clip_fraction": r[4] / n, "value_mean": r[5] / n,
               "returns_mean": r[6] / n, "value_error_mean": r[7] / n, "value_error_max": r[9]}
        if "sha_masks" in fx.files and o["avg_valid_actions"] > 0:
            dev["avg_valid_actions"] = r[11] / n
            dev["entropy_valid_pct"] = r[12] / r[13] if r[13] > 0 else 0.0
        floor = {"policy_loss": pl_mag, "value_mean": abs(o["value_error_mean"]) + abs(o["returns_mean"]),
                 "returns_mean": abs(o["value_error_mean"]) + abs(o["returns_mean"])}
        absf = {"approx_kl": 2.0 ** -24 / np.sqrt(mb), "clip_fraction": 4.0 / mb}
        rel = {f: abs(float(dev[f]) - o[f]) / max(RTOL * max(abs(o[f]), floor.get(f, 0.0)), absf.get(f, 0.0), 1e-37)
               for f in dev}
        f = max(rel, key=rel.get)
        worst.append((k, f, round(rel[f], 3)))
        if rel[f] > 1.0 and k < first_epoch_rows:
            bad.append((k, f, float(dev[f]), o[f]))
    print(f"\nper-minibatch worst error / bar (oracle trajectory): {worst}")
    assert not bad, bad


@pytest.mark.parametrize("case", list(CASES))
def test_bench_path_matches_fullsize_oracle(case):
    fx = np.load(os.path.join(GOLDEN, f"full_{case}.npz"))
    assert json.loads(str(fx["config"])) == CASES[case]
    c = dict(CASES[case])
    preset, init_seed = c.pop("preset"), c.pop("init_seed")
    cfg = bppo.make_config(preset, **c)
    N, T = cfg["num_envs"], cfg["num_steps"]
    params = bppo.orthogonal_init(cfg, seed=init_seed)
    assert sha(params) == str(fx["init_sha"]), "orthogonal_init regenerated different weights"
    tr = bppo.Trainer(cfg, params=params)
    try:
        (m,), _ = tr.train_updates(1)
        ctx = tr.ctx
        # rollout: RNG position, episodes, bit-exact buffers
        assert m["rng_word_pos"] == int(fx["rng_rollout"])
        assert m["episodes"] == int(fx["episodes"])
        bad = [b for b, dt in _exact_buffers(cfg) if sha(ctx.buffer(b, dt)) != str(fx["sha_" + b])]
        assert not bad, f"buffers differ from the oracle: {bad}"
        if cfg["env"] == "cartpole":
            mean, m2, cnt = ctx.obs_norm()
            assert cnt == float(fx["obs_norm_count"])
            np.testing.assert_allclose(mean, fx["obs_norm_mean"], rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(m2, fx["obs_norm_m2"], rtol=1e-10)
            mvc, rets = ctx.ret_norm()
            assert sha(rets) == str(fx["sha_ret_norm_returns"])
            np.testing.assert_allclose(mvc, fx["ret_norm"], rtol=1e-12)
            for b, rtol in (("rewards", 2e-7), ("advantages", RTOL), ("returns", RTOL)):
                x = ctx.buffer(b)
                s = int(fx["sample_stride"])
                np.testing.assert_allclose(x[7::s], fx["sample_" + b], rtol=rtol, atol=rtol * 1e-2, err_msg=b)
                rs = x.reshape(T, N).astype(np.float64).sum(axis=1)
                np.testing.assert_allclose(rs, fx["rowsum_" + b], rtol=rtol, atol=rtol * N * 1e-2, err_msg=b)
        else:
            assert sha(ctx.buffer("last_v_pp")) == str(fx["sha_last_v_pp"])
        # the update: shuffle chain, permutation, metrics, parameters
        assert ctx.rng_pos() == int(fx["rng_update"])
        assert m["num_updates"] == int(fx["num_updates"]) and m["epochs_run"] == int(fx["epochs_run"])
        assert sha(ctx.buffer("perm", np.uint32)) == str(fx["sha_perm"])
        om = dict(zip(METRICS, (float(v) for v in fx["metrics"])))
        pl_mag = summand_magnitude(ctx.buffer("advantages"))
        bad = []
        for k in METRICS:
            d, o = float(m[k]), om[k]
            if k == "explained_variance":
                if abs(d - float(fx["ev_exact"])) > 1e-6:
                    bad.append((k, d, float(fx["ev_exact"])))
                continue
            tol = RTOL * max(abs(o), _floor(k, om, pl_mag))
            if k == "clip_fraction":
                # a count: rows whose ratio sits within rounding of 1 +- eps flip when the
                # later minibatches' parameters differ in the last bits; allow 4 per minibatch
                tol = max(tol, 4.0 / (N * T // cfg["num_minibatches"]))
            if not abs(d - o) <= tol:
                bad.append((k, d, o))
        assert not bad, bad
        if "mb_log" in fx.files:
            _check_minibatch_rows(ctx.minibatch_rows(), fx, N * T // cfg["num_minibatches"], pl_mag,
                                  cfg["num_minibatches"])
        p = tr.model.get_params()
        # parameters after E x M Adam steps: Adam's m/sqrt(v) turns last-bit gradient
        # differences of near-zero entries into differences of up to ~lr per step, so a
        # rare entry leaves the single-step bound (CfgC, 24 steps: 1 of 16384 sampled at
        # 3.5e-5); at most 0.1 % may, and none by more than 1 % of lr per step
        ps, po = p[fx["param_idx"]], fx["param_sample"]
        off = ~np.isclose(ps, po, rtol=PARAM_RTOL, atol=PARAM_ATOL)
        lr = bppo.schedule_get(cfg["learning_rate"], 0)
        assert off.mean() <= 1e-3, (off.sum(), off.size)
        assert np.abs(ps - po).max() <= 0.01 * lr * int(fx["num_updates"]), np.abs(ps - po).max()
        deltas, o = [], 0
        for sz in _layer_sizes(cfg):
            deltas.append(np.abs(p[o:o + sz].astype(np.float64) - params[o:o + sz].astype(np.float64)).sum())
            o += sz
        np.testing.assert_allclose(deltas, fx["tensor_abs_delta"], rtol=1e-4, atol=1e-9)
    finally:
        tr.close()


def _net_desc(cfg):
    D, A, _, G = bppo.host.ENV_DIMS[cfg["env"]]
    relu = cfg["activation"] == "relu"
    if cfg["network_type"] == "ctde":
        return O.ctde_desc(D, G, A, cfg["hidden_size"], cfg["num_hidden"], cfg["critic_hidden_size"],
                           cfg["critic_num_hidden"], relu)
    return O.mlp_desc(D, A, cfg["hidden_size"], cfg["num_hidden"], relu)


@pytest.mark.parametrize("case", list(CASES))
def test_bench_minibatches_from_device_parameters(case):
    """Every minibatch of one benched update, recomputed by the oracle FROM THE PARAMETERS THE
    DEVICE RAN IT WITH (bppo_debug_record_params), on the rows of that minibatch (the epoch's
    permutation, "perm_ep:<e>"): the device's statistics (bppo_minibatch_rows) against
    or_minibatch_loss_grad's (ppo.rs:1923-1988; forward + loss, per-minibatch advantage
    normalization ppo.rs:1905-1913) at 1e-5 with the update metrics' floors.  This pins the
    arithmetic the bench runs at the sizes it runs -- CfgB's 2,097,152-row minibatches
    (k_minibatch_split<true>: exact forward, split backward; then k_minibatch_split), CfgC's 262,144 and CfgD's 524,288 (the first
    minibatch's exact forward, then the split-bf16 GEMMs) -- without the parameter drift that
    separates the two trajectories after a few Adam steps (the fixture comparison above).
    CfgD: the first two minibatches of every epoch (the oracle's forward of a 524,288-row
    CTDE minibatch takes ~6 s on the box)."""
    fx = np.load(os.path.join(GOLDEN, f"full_{case}.npz"))
    assert json.loads(str(fx["config"])) == CASES[case]
    c = dict(CASES[case])
    preset, init_seed = c.pop("preset"), c.pop("init_seed")
    cfg = bppo.make_config(preset, **c)
    N, T = cfg["num_envs"], cfg["num_steps"]
    B, E, M = N * T, cfg["num_epochs"], cfg["num_minibatches"]
    params = bppo.orthogonal_init(cfg, seed=init_seed)
    tr = bppo.Trainer(cfg, params=params)
    try:
        ctx = tr.ctx
        rec = ctx.record_params(E * M)
        (m,), _ = tr.train_updates(1)
        rows = ctx.minibatch_rows()
        assert len(rows) == E * M or cfg["target_kl"] is not None
        D, A, _, G = bppo.host.ENV_DIMS[cfg["env"]]
        obs = ctx.buffer("obs").reshape(B, D)
        priv = ctx.buffer("priv").reshape(B, G) if cfg["network_type"] == "ctde" else None
        masks = ctx.buffer("masks").reshape(B, A) if cfg["env"] != "cartpole" else None
        act = ctx.buffer("actions", np.int32)
        logp, val, ret, adv = (ctx.buffer(k) for k in ("log_probs", "values", "returns", "advantages"))
        desc = _net_desc(cfg)
        pc = O.ppo_cfg(num_epochs=1, num_minibatches=1, clip=cfg["clip_epsilon"], value_coef=cfg["value_coef"],
                       clip_value=bool(cfg.get("clip_value")))
        ent = bppo.schedule_get(cfg["entropy_coef"], 0)
        base, rem = B // M, B % M
        pl_mag = summand_magnitude(adv)
        perms, worst, bad = {}, [], []
        for k, r in enumerate(rows):
            e, mb = divmod(k, M)
            if case == "cfgD" and mb >= 2:
                continue        # ~6 s of oracle forward per 524,288-row minibatch: two per epoch
            if e not in perms:
                perms[e] = ctx.buffer(f"perm_ep:{e}", np.uint32)
            start = mb * base + min(mb, rem)
            sz = base + (1 if mb < rem else 0)
            idx = perms[e][start:start + sz]
            advn = np.zeros(sz, np.float32)
            st = [C.c_float() for _ in range(4)]
            O.lib().or_normalize_advantages(np.ascontiguousarray(adv[idx]), sz, advn, *[C.byref(x) for x in st])
            o = O.minibatch_stats(desc, rec[k], obs[idx], None if priv is None else priv[idx], act[idx], logp[idx],
                                  advn, ret[idx], val[idx], None if masks is None else masks[idx], pc, ent)
            n = float(r[10])
            assert n == sz, (k, n, sz)
            dev = {"policy_loss": r[0] / n, "value_loss": 0.5 * r[1] / n, "entropy": r[2] / n,
                   "approx_kl": r[3] / n, "clip_fraction": r[4] / n, "value_mean": r[5] / n,
                   "returns_mean": r[6] / n, "value_error_mean": r[7] / n, "value_error_max": r[9]}
            if masks is not None:
                dev["avg_valid_actions"] = r[11] / n
            floor = {"policy_loss": pl_mag, "value_mean": abs(o["value_error_mean"]) + abs(o["returns_mean"]),
                     "returns_mean": abs(o["value_error_mean"]) + abs(o["returns_mean"])}
            absf = {"approx_kl": 2.0 ** -24 / np.sqrt(sz), "clip_fraction": 4.0 / sz}
            rel = {f: abs(float(dev[f]) - o[f]) / max(RTOL * max(abs(o[f]), floor.get(f, 0.0)), absf.get(f, 0.0), 1e-37)
                   for f in dev}
            f = max(rel, key=rel.get)
            worst.append((k, f, round(rel[f], 3)))
            if rel[f] > 1.0:
                bad.append((k, f, float(dev[f]), o[f]))
        print(f"\n{case}: per-minibatch worst error / bar from the device's parameters: {worst}")
        assert not bad, bad
    finally:
        tr.close()


def test_updates_without_injection_action_agreement():
    """K = 8 CartPole updates (2x64 relu, 4 x 4 minibatches, both normalizers) at
    N = 2,048, T = 128 on both sides with NOTHING injected between them: the device
    runs each through bppo_train_steps (the bench's call; its pipelined form equals
    one call per update bit for bit, test_gpu_scale.py), the oracle sequentially.  The first
    rollout is bit-exact and the first update within the metric tolerance (as above);
    after that the parameters differ in the last bits (gradient reduction order), so
    the per-update share of identical actions is reported (measured r03 with the 32-row
    minibatch kernel: identical for 6 updates, then 99.97 % / 99.7 %; with the 16-row
    kernel's gradient order: identical for 4, then 99.99 / 99.92 / 99.6 / 98.9 %; the
    metrics drift from 3e-9 to 1e-2 .. 1e-1 relative by update 8 -- trajectories of a
    chaotic system from last-bit parameter differences, whose divergence rate is the
    system's, not the kernel's).  The first 4 updates must keep >= 99.9 % of the
    actions and every update >= 98 %."""
    N, T, K = 2048, 128, 8
    cfg = bppo.make_config("cartpole", num_envs=N, num_steps=T, seed=42)
    params = bppo.orthogonal_init(cfg, seed=1)
    ot = O.Trainer(oracle_train_cfg(cfg), params)
    tr = bppo.Trainer(cfg, params=params)
    try:
        agree, first_diff, worst = [], None, []
        for k in range(K):
            (m,), _ = tr.train_updates(1)
            ot.collect(); ot.gae()
            da, oa = tr.buffer.actions.reshape(-1), ot.buffer("actions", np.int32)
            agree.append(float((da == oa).mean()))
            if first_diff is None and not np.array_equal(da, oa):
                first_diff = k
            om = ot.update()
            mag = summand_magnitude(ot.buffer("advantages"))
            rel = max(abs(float(m[q]) - om[q]) / max(abs(om[q]), _floor(q, om, mag), 1e-6)
                      for q in METRICS if q != "explained_variance")
            worst.append(rel)
        print(f"\naction agreement per update: {agree}\nfirst differing rollout: {first_diff}\n"
              f"worst metric rel. difference per update: {[f'{w:.1e}' for w in worst]}")
        assert agree[0] == 1.0 and worst[0] <= RTOL
        assert min(agree[:4]) >= 0.999 and min(agree) >= 0.98, agree
    finally:
        tr.close(); ot.close()
