"""The stages of bppo_ppo_update (csrc/train_loop.hip) at the smallest shapes that reach each
of its paths: after one update, the metric fold (bppo_debug_fold_metrics) applied to the
update's own rows (bppo_minibatch_rows) reproduces the returned bppo_update_metrics bit for
bit, and the KL early stop leaves the epochs, minibatches and RNG position the oracle's
leaves.  The rows folded here are the host copy the update itself folded, so the fold check
pins the fold's arguments and the export on each path, not how a row policy read the rows off
the device: that rests on the oracle comparison here and on the metric parity tests
(test_gpu_wide.py, test_gpu_fullsize.py).  The explained variance is left out of the
comparison: its sums are not in the rows."""
import ctypes as C

import numpy as np
import pytest

import bppo
import bppo._lib as L
import oracle_ffi as O
from bppo.host import shaping_schedule

pytestmark = pytest.mark.gpu

C4_KIND, C4_OBS, C4_ACTIONS, C4_PLAYERS = 1, 86, 7, 2
C4 = dict(num_envs=32, num_steps=8, num_epochs=3, num_minibatches=2, hidden_size=64, target_kl=1e-9, seed=42)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return bits(np.float32(a)).tolist() == bits(np.float32(b)).tolist()


def assert_fold_reproduces(tr, m):
    """fold(the update's rows) == the update's metrics, every field but explained_variance"""
    cfg, rows = tr.cfg, tr.ctx.minibatch_rows()
    assert rows.shape[0] == m["num_updates"]
    # B and ev4 feed the explained variance only, which is not compared: T * N stands in for the
    # opponent pool's learner-row count too
    fa = L.FoldArgs(value_coef=cfg["value_coef"], ent_coef=bppo.schedule_get(cfg["entropy_coef"], 0),
                    A=tr.ctx.num_actions, env_kind=tr.ctx.struct.env_kind, B=tr.ctx.T * tr.ctx.N,
                    epochs_run=m["epochs_run"], normalize_values=0,
                    pa_rescale_mag=np.nan)                 # PopArt off: the reference's None (ppo.rs:1799-1804)
    out = L.UpdateMetrics()
    assert L.lib().bppo_debug_fold_metrics(rows.ctypes.data, rows.shape[0], C.byref(fa), C.byref(out)) == L.OK
    for k in L.METRIC_NAMES + L.POPART_METRICS:
        if k != "explained_variance":
            assert same_bits(getattr(out, k), m[k]), (k, getattr(out, k), m[k])
    assert (out.num_updates, out.epochs_run) == (m["num_updates"], m["epochs_run"])


def test_deferred_rows_cartpole():
    """no KL stop, one rank: the minibatches run back to back and the rows are read once"""
    cfg = bppo.make_config("cartpole", num_envs=64, num_steps=16, num_epochs=2, num_minibatches=2,
                           hidden_size=64, num_hidden=2, activation="relu")
    tr = bppo.Trainer(cfg, init_seed=3)
    try:
        m = tr.train_update()
        assert (m["num_updates"], m["epochs_run"]) == (4, 2)
        assert_fold_reproduces(tr, m)
    finally:
        tr.close()


def c4_pair():
    cfg = bppo.make_config("connect_four", **C4)
    params = bppo.orthogonal_init(cfg, seed=5)
    tr = bppo.Trainer(cfg, params=params)
    ocfg = O.train_cfg(env_kind=C4_KIND, num_envs=cfg["num_envs"], num_steps=cfg["num_steps"], seed=cfg["seed"],
                       hidden=cfg["hidden_size"], num_hidden=cfg["num_hidden"], relu=cfg["activation"] == "relu",
                       normalize_obs=bool(cfg["normalize_obs"]), normalize_returns=bool(cfg["normalize_returns"]),
                       gamma=cfg["gamma"], gae_lambda=cfg["gae_lambda"], lr=bppo.schedule_get(cfg["learning_rate"], 0),
                       ent_coef=bppo.schedule_get(cfg["entropy_coef"], 0),
                       reward_shaping=bppo.schedule_get(shaping_schedule(cfg), 0), num_epochs=cfg["num_epochs"],
                       num_minibatches=cfg["num_minibatches"], clip=cfg["clip_epsilon"], value_coef=cfg["value_coef"],
                       target_kl=cfg["target_kl"])
    return cfg, params, tr, O.Trainer(ocfg, params)


def opponent_seats(cfg, n_opp, K, seed=3):
    rng = np.random.default_rng(seed)
    params = np.stack([bppo.orthogonal_init(cfg, seed=100 + k) for k in range(K)])
    lp = rng.integers(0, C4_PLAYERS, n_opp).astype(np.int32)
    po = np.full((n_opp, C4_PLAYERS), -1, np.int32)
    for e in range(n_opp):
        po[e, 1 - lp[e]] = rng.integers(0, K)
    return params, lp, po, rng.integers(0, K, C4_PLAYERS - 1).astype(np.int32)


@pytest.mark.parametrize("pool", [False, True])
def test_immediate_rows_kl_stop_connect_four(pool):
    """target_kl = 1e-9: every row is read as its minibatch ends and the second one stops the
    update (the first runs the rollout's parameters: KL 0).  pool: the learner rows only, each
    epoch's permutation from the sequential host walk instead of the shuffle engine."""
    cfg, params, tr, ot = c4_pair()
    try:
        if pool:
            op, lp, po, co = opponent_seats(cfg, n_opp=20, K=2)
            tr.ctx.set_opponents(op, [None, None], 20, lp, po, co)
            ot.set_opponents(op, [None, None], 20, lp, po.reshape(-1), co)
        bppo.collect_rollouts(tr.ctx); ot.collect()
        assert tr.ctx.rng_pos() == ot.rng_pos()
        bppo.compute_gae(tr.ctx); ot.gae()
        m = bppo.ppo_update(tr.ctx, bppo.schedule_get(cfg["learning_rate"], 0), bppo.schedule_get(cfg["entropy_coef"], 0))
        om = ot.update()
        assert m["epochs_run"] < 3 and m["num_updates"] < 6            # it stopped
        assert (m["epochs_run"], m["num_updates"]) == (om["epochs_run"], om["num_updates"])
        assert tr.ctx.rng_pos() == ot.rng_pos()                        # only the started epochs drew words
        assert_fold_reproduces(tr, m)
    finally:
        tr.close(); ot.close()


def test_pipelined_equals_sequential_cartpole():
    """the prefetch tail: train_updates(3) is three train_update() calls, bit for bit"""
    cfg = bppo.make_config("cartpole", num_envs=64, num_steps=16, num_epochs=2, num_minibatches=2,
                           hidden_size=64, num_hidden=2, activation="relu", seed=13)
    a, b = bppo.Trainer(cfg, init_seed=4), bppo.Trainer(cfg, init_seed=4)
    try:
        seq = [a.train_update() for _ in range(3)]
        pip, _ = b.train_updates(3)
        for ma, mb in zip(seq, pip):
            for k, v in ma.items():
                assert same_bits(v, mb[k]) or (np.isnan(v) and np.isnan(mb[k])), k
        assert bits(a.model.get_params()).tolist() == bits(b.model.get_params()).tolist()
        assert a.ctx.rng_pos() == b.ctx.rng_pos()
    finally:
        a.close(); b.close()
