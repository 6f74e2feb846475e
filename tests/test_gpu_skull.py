"""Skull (envs/skull.rs) on the device vs the oracle restatement (oracle/skull.c,
pinned by the reference's own Skull tests in tests/test_oracle_skull.py).

Bit-exact: VecEnv transitions for 2/4/6 players (observations, privileged obs,
masks, acting players, rewards incl. shaping and tie-averaged placement
rewards, dones, episode records, the env RNG's lose_coaster draws), rollouts
(masked Gumbel-max actions, log-probs, values), multi-player GAE over the 6-seat
player axis.  The update: every UpdateMetrics field within 1e-5 relative and
parameters within rtol 1e-4 / atol 2e-5 (tests/parity_util.py), as for the
other multi-player envs.  An action outside the mask (a panic in the reference)
is BPPO_ERR_ARG.  With the observation / return normalizers on (3, 5 and 6 seats, self-play
and opponent pool), PopArt, and a checkpoint of the 6-seat return normalizer: the bars of
tests/test_gpu_wide.py and tests/test_gpu_popart.py."""
import numpy as np
import pytest

import bppo
import oracle_ffi as O
from parity_util import assert_metrics_close, assert_params_close

pytestmark = pytest.mark.gpu
D, A, P, G = 135, 33, 6, 200


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("players,ctde,shaping", [(4, True, 0.1), (2, False, 0.0), (6, True, 0.0), (3, False, 0.05)])
def test_vecenv_matches_oracle(players, ctde, shaping):
    N = 256
    cfg = bppo.make_config("skull_ctde" if ctde else "skull", num_envs=N, num_steps=4, player_count=players,
                           reward_shaping_coef=shaping)
    ctx = bppo.Context(cfg)
    ve = bppo.VecEnv.new(ctx)
    ov = O.lib().or_vecenv_new_np(O.ENV_SKULL, N, cfg["seed"], players)
    O.lib().or_vecenv_set_shaping(ov, shaping)
    obs_o = np.zeros(N * D, np.float32); m_o = np.zeros(N * A, np.uint8); pl_o = np.zeros(N, np.int32)
    g_o = np.zeros(N * G, np.float32); rw = np.zeros(N * P, np.float32); dn = np.zeros(N, np.uint8)
    eps = (O.Episode * N)()
    rng = np.random.default_rng(3)
    n_done = 0
    for t in range(500):
        O.lib().or_vecenv_get_obs(ov, obs_o)
        O.lib().or_vecenv_get_masks(ov, m_o)
        O.lib().or_vecenv_get_players(ov, pl_o)
        assert np.array_equal(ve.get_observations(), obs_o), t
        assert np.array_equal(ve.get_action_masks(), m_o.astype(bool)), t
        assert np.array_equal(ve.get_current_players(), pl_o), t
        if ctde:
            O.lib().or_vecenv_get_priv(ov, g_o)
            assert np.array_equal(ve.get_privileged_obs(), g_o), t
        m = m_o.reshape(N, A).astype(bool)
        a = np.array([rng.choice(np.flatnonzero(row)) for row in m], np.int32)
        o, r, d, ep = ve.step(a)
        ne = O.lib().or_vecenv_step(ov, a, obs_o, rw, dn, eps, N)
        assert np.array_equal(_bits(o), _bits(obs_o)), t
        assert np.array_equal(_bits(r.reshape(-1)), _bits(rw)), t
        assert np.array_equal(d, dn.astype(bool)), t
        assert len(ep) == ne
        for i, e in enumerate(ep):
            assert e["env_index"] == eps[i].env_index and e["length"] == eps[i].length
            assert np.array_equal(_bits(e["total_rewards"]), _bits(eps[i].total_rewards[:P]))
        n_done += int(d.sum())
    assert n_done > 20 and O.lib().or_vecenv_invalid(ov) == 0
    # an action outside the mask: the reference panics (skull.rs:1113-1128)
    m = ve.get_action_masks().reshape(N, A)
    a = np.array([np.flatnonzero(row)[0] for row in m], np.int32)
    a[0] = int(np.flatnonzero(~m[0])[0])
    with pytest.raises(bppo.BppoError):
        ve.step(a)
    O.lib().or_vecenv_free(ov)
    ctx.close()


def test_player_count_validation():
    for bad in (1, 7):
        with pytest.raises(bppo.BppoError):
            bppo.Context(bppo.make_config("skull", num_envs=8, num_steps=4, player_count=bad))


def _pair(N, T, ctde, players, seed=42, **kw):
    cfg = bppo.make_config("skull_ctde" if ctde else "skull", num_envs=N, num_steps=T, seed=seed,
                           player_count=players, hidden_size=64, num_hidden=2, critic_hidden_size=64,
                           critic_num_hidden=2, **kw)
    params = bppo.orthogonal_init(cfg, seed=5)
    tr = bppo.Trainer(cfg, params=params)
    ocfg = O.train_cfg(env_kind=O.ENV_SKULL, num_envs=N, num_steps=T, seed=seed, hidden=cfg["hidden_size"],
                       num_hidden=cfg["num_hidden"], ctde=ctde, relu=True,
                       critic_hidden=cfg["critic_hidden_size"] if ctde else 0,
                       critic_num_hidden=cfg["critic_num_hidden"] if ctde else 0,
                       normalize_obs=bool(cfg["normalize_obs"]), normalize_returns=bool(cfg["normalize_returns"]),
                       normalize_values=bool(cfg.get("normalize_values", False)), gamma=cfg["gamma"], gae_lambda=cfg["gae_lambda"],
                       lr=bppo.schedule_get(cfg["learning_rate"], 0), ent_coef=bppo.schedule_get(cfg["entropy_coef"], 0),
                       reward_shaping=cfg["reward_shaping_coef"], num_epochs=cfg["num_epochs"],
                       num_minibatches=cfg["num_minibatches"], clip=cfg["clip_epsilon"], value_coef=cfg["value_coef"],
                       target_kl=cfg["target_kl"], player_count=players)
    return cfg, tr, O.Trainer(ocfg, params)


def _cmp_rollout(tr, ot, ctde, rew_rtol=0.0):
    b = tr.buffer
    assert np.array_equal(b.acting_players.reshape(-1), ot.buffer("players", np.int32))
    assert np.array_equal(_bits(b.observations.reshape(-1)), _bits(ot.buffer("obs")))
    assert np.array_equal(b.action_masks.reshape(-1), ot.buffer("masks"))
    if ctde:
        assert np.array_equal(_bits(b.privileged_obs.reshape(-1)), _bits(ot.buffer("priv")))
    assert np.array_equal(b.actions.reshape(-1), ot.buffer("actions", np.int32))
    assert np.array_equal(_bits(b.values.reshape(-1)), _bits(ot.buffer("values")))
    assert np.array_equal(_bits(b.log_probs.reshape(-1)), _bits(ot.buffer("log_probs")))
    assert np.array_equal(b.dones.reshape(-1), ot.buffer("dones"))
    if rew_rtol:
        # return normalizer: f64 Welford block scan vs the sequential update (merge order),
        # as tests/test_gpu_wide.py's _cmp_rollout
        np.testing.assert_allclose(b.rewards.reshape(-1), ot.buffer("rewards"), rtol=rew_rtol, atol=0)
        np.testing.assert_allclose(b.all_rewards.reshape(-1), ot.buffer("all_rewards"), rtol=rew_rtol, atol=0)
    else:
        assert np.array_equal(_bits(b.rewards.reshape(-1)), _bits(ot.buffer("rewards")))
        assert np.array_equal(_bits(b.all_rewards.reshape(-1)), _bits(ot.buffer("all_rewards")))
    assert tr.ctx.rng_pos() == ot.rng_pos()


@pytest.mark.parametrize("N,T,ctde,players", [(64, 32, True, 4), (48, 24, False, 6), (1024, 16, True, 3)])
def test_rollout_gae_update_second_rollout(N, T, ctde, players):
    cfg, tr, ot = _pair(N, T, ctde, players)
    info = bppo.collect_rollouts(tr.ctx)
    n_eps = ot.collect()
    _cmp_rollout(tr, ot, ctde)
    assert info.episodes == n_eps
    bppo.compute_gae(tr.ctx); ot.gae()
    assert np.array_equal(_bits(tr.ctx.buffer("last_v_pp")), _bits(ot.buffer("last_v_pp")))
    assert np.array_equal(_bits(tr.buffer.advantages.reshape(-1)), _bits(ot.buffer("advantages")))
    assert np.array_equal(_bits(tr.buffer.returns.reshape(-1)), _bits(ot.buffer("returns")))
    m = bppo.ppo_update(tr.ctx, bppo.schedule_get(cfg["learning_rate"], 0), bppo.schedule_get(cfg["entropy_coef"], 0))
    om = ot.update()
    assert tr.ctx.rng_pos() == ot.rng_pos()
    assert_metrics_close(m, om, values=ot.buffer("values"), returns=ot.buffer("returns"), advantages=ot.buffer("advantages"))
    assert_params_close(tr.model.get_params(), ot.params())
    tr.model.set_params(ot.params())
    bppo.collect_rollouts(tr.ctx); ot.collect()
    _cmp_rollout(tr, ot, ctde)
    tr.close(); ot.close()


@pytest.mark.parametrize("players,ctde", [(4, True), (5, False)])
def test_opponent_pool_rollout_update(players, ctde):
    """collect_rollouts_with_opponents over the seated players (EnvState with
    main.rs:552's actual_player_count): seat draws, opponent batches, learner-only
    update -- bit-exact rollouts, update within the usual tolerances."""
    N, T, n_opp, K = 48, 12, 32, 2
    cfg, tr, ot = _pair(N, T, ctde, players)
    rng = np.random.default_rng(7)
    params = np.stack([bppo.orthogonal_init(cfg, seed=100 + k) for k in range(K)])
    lp = rng.integers(0, players, n_opp).astype(np.int32)
    po = np.full((n_opp, players), -1, np.int32)
    for e in range(n_opp):
        for p in range(players):
            if p != lp[e]:
                po[e, p] = rng.integers(0, K)
    co = rng.integers(0, K, players - 1).astype(np.int32)
    tr.ctx.set_opponents(params, [None] * K, n_opp, lp, po, co)
    ot.set_opponents(params, [None] * K, n_opp, lp, po.reshape(-1), co)
    for _ in range(2):
        bppo.collect_rollouts(tr.ctx); ot.collect()
        _cmp_rollout(tr, ot, ctde)
        assert np.array_equal(tr.ctx.buffer("valid"), ot.buffer("valid"))
        l1, p1 = tr.ctx.opponent_envs()
        l2, p2 = ot.opponent_envs(n_opp, players)
        assert np.array_equal(l1, l2) and np.array_equal(p1.reshape(-1), p2)
        bppo.compute_gae(tr.ctx); ot.gae()
        assert np.array_equal(_bits(tr.buffer.advantages.reshape(-1)), _bits(ot.buffer("advantages")))
        m = bppo.ppo_update(tr.ctx, bppo.schedule_get(cfg["learning_rate"], 0),
                            bppo.schedule_get(cfg["entropy_coef"], 0))
        om = ot.update()
        assert tr.ctx.rng_pos() == ot.rng_pos()
        vm = ot.buffer("valid") > 0.5
        assert_metrics_close(m, om, values=ot.buffer("values")[vm], returns=ot.buffer("returns")[vm], advantages=ot.buffer("advantages")[vm])
        assert_params_close(tr.model.get_params(), ot.params())
        tr.model.set_params(ot.params())
    tr.close(); ot.close()


# ---------------------------------------------------------- normalizers ---
# The reference lets normalize_returns be switched on for any env (config.rs:243-249): one
# rolling return per (env, seat) over Skull's 6 seats.  Seats 4 and 5 act only at 5 and 6
# players -- where k_rn_returns_mp used to fold them onto seat 3.  Skull pays at a game's end
# only, on a step that resets the acting seat's return, so without reward shaping every rolling
# return stays 0 and no seat can be told from another: these cases run with round rewards
# (reward_shaping_coef), and check that the seats' returns are there.
SHAPING = 0.1


def _seats_hold_returns(orets, N, players):
    r = orets.reshape(N, P)
    assert (r[:, :players] != 0).any(axis=0).all() and not r[:, players:].any()


def _cmp_norm_state(tr, ot, N, T=None):
    m, v, c = tr.ctx.obs_norm()
    mo, vo, co = ot.obs_norm_state(D)
    assert c == co and (T is None or c == N * T)
    np.testing.assert_allclose(m, mo, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(v, vo, rtol=1e-10, atol=1e-12)
    mvc, rets = tr.ctx.ret_norm()
    omvc, orets = ot.ret_norm_state(returns=True)
    assert rets.size == orets.size == N * P
    bad = np.argwhere(rets.reshape(N, P) != orets.reshape(N, P))
    assert bad.size == 0, "returns differ in %d slots, seats %s" % (len(bad), sorted(set(bad[:, 1].tolist())))
    assert mvc[2] == omvc[2]
    np.testing.assert_allclose(mvc, omvc, rtol=1e-12)
    return omvc, orets


@pytest.mark.parametrize("N,T,ctde,players", [(48, 24, False, 6), (64, 20, True, 5), (64, 17, False, 3)])
def test_normalizers_rollout_update_second_rollout(N, T, ctde, players):
    """the flow of tests/test_gpu_wide.py's test of the same name, on 3, 5 and 6 seats"""
    cfg, tr, ot = _pair(N, T, ctde, players, normalize_obs=True, normalize_returns=True, reward_shaping_coef=SHAPING)
    bppo.collect_rollouts(tr.ctx); ot.collect()
    _cmp_rollout(tr, ot, ctde, rew_rtol=2e-7)
    acted = np.bincount(ot.buffer("players", np.int32), minlength=P)
    assert (acted[:players] > 0).all() and not acted[players:].any()      # every seated player acted
    omvc, orets = _cmp_norm_state(tr, ot, N, T)
    assert omvc[2] == N * T
    _seats_hold_returns(orets, N, players)
    bppo.compute_gae(tr.ctx); ot.gae()
    np.testing.assert_allclose(tr.buffer.advantages.reshape(-1), ot.buffer("advantages"), rtol=1e-5, atol=1e-6)
    m = bppo.ppo_update(tr.ctx, bppo.schedule_get(cfg["learning_rate"], 0), bppo.schedule_get(cfg["entropy_coef"], 0))
    om = ot.update()
    assert_metrics_close(m, om, values=ot.buffer("values"), returns=ot.buffer("returns"), advantages=ot.buffer("advantages"))
    assert_params_close(tr.model.get_params(), ot.params())
    # second rollout from the oracle's parameters and normalizer state
    tr.model.set_params(ot.params())
    tr.ctx.set_obs_norm(*ot.obs_norm_state(D))
    tr.ctx.set_ret_norm(omvc, orets)
    bppo.collect_rollouts(tr.ctx); ot.collect()
    _cmp_rollout(tr, ot, ctde, rew_rtol=2e-7)
    _cmp_norm_state(tr, ot, N)
    tr.close(); ot.close()


def test_opponent_pool_with_normalizers_five_players():
    """test_opponent_pool_rollout_update with both normalizers on and n_opp < N: rows acted
    by an opponent move their seat's rolling return but stay out of the variance statistics"""
    players, ctde = 5, False
    N, T, n_opp, K = 48, 12, 32, 2
    cfg, tr, ot = _pair(N, T, ctde, players, normalize_obs=True, normalize_returns=True, reward_shaping_coef=SHAPING)
    rng = np.random.default_rng(7)
    params = np.stack([bppo.orthogonal_init(cfg, seed=100 + k) for k in range(K)])
    lp = rng.integers(0, players, n_opp).astype(np.int32)
    po = np.full((n_opp, players), -1, np.int32)
    for e in range(n_opp):
        for p in range(players):
            if p != lp[e]:
                po[e, p] = rng.integers(0, K)
    co = rng.integers(0, K, players - 1).astype(np.int32)
    tr.ctx.set_opponents(params, [None] * K, n_opp, lp, po, co)
    ot.set_opponents(params, [None] * K, n_opp, lp, po.reshape(-1), co)
    n_valid = 0
    for rnd in range(2):
        if rnd:                                # layered: the oracle's normalizer state
            tr.ctx.set_obs_norm(*ot.obs_norm_state(D))
            tr.ctx.set_ret_norm(*ot.ret_norm_state(returns=True))
        bppo.collect_rollouts(tr.ctx); ot.collect()
        _cmp_rollout(tr, ot, ctde, rew_rtol=2e-7)
        assert np.array_equal(tr.ctx.buffer("valid"), ot.buffer("valid"))
        v = ot.buffer("valid").reshape(T, N)
        assert v[:, n_opp:].min() == 1.0 and 0.0 < v[:, :n_opp].mean() < 1.0
        l1, p1 = tr.ctx.opponent_envs()
        l2, p2 = ot.opponent_envs(n_opp, players)
        assert np.array_equal(l1, l2) and np.array_equal(p1.reshape(-1), p2)
        mvc, rets = tr.ctx.ret_norm()
        omvc, orets = ot.ret_norm_state(returns=True)
        n_valid += int((v > 0.5).sum())
        assert mvc[2] == omvc[2] == n_valid < (rnd + 1) * N * T          # learner rows only
        assert np.array_equal(rets, orets)
        if rnd:
            _seats_hold_returns(orets, N, players)
        np.testing.assert_allclose(mvc, omvc, rtol=1e-12)
        bppo.compute_gae(tr.ctx); ot.gae()
        np.testing.assert_allclose(tr.buffer.advantages.reshape(-1), ot.buffer("advantages"), rtol=1e-5, atol=1e-6)
        m = bppo.ppo_update(tr.ctx, bppo.schedule_get(cfg["learning_rate"], 0),
                            bppo.schedule_get(cfg["entropy_coef"], 0))
        om = ot.update()
        assert tr.ctx.rng_pos() == ot.rng_pos()
        vm = ot.buffer("valid") > 0.5
        assert_metrics_close(m, om, values=ot.buffer("values")[vm], returns=ot.buffer("returns")[vm], advantages=ot.buffer("advantages")[vm])
        assert_params_close(tr.model.get_params(), ot.params())
        tr.model.set_params(ot.params())
    tr.close(); ot.close()


@pytest.mark.parametrize("N,T,ctde,players", [(48, 16, False, 6), (64, 12, True, 4)])
def test_popart_skull(N, T, ctde, players):
    """normalize_values on Skull: tests/test_gpu_popart.py's three layered rounds"""
    from test_gpu_popart import _cmp_wide, _rounds
    cfg, tr, ot = _pair(N, T, ctde, players, normalize_values=True)
    _rounds(cfg, tr, ot, _cmp_wide)
    tr.close(); ot.close()


def test_checkpoint_keeps_six_player_returns(tmp_path):
    """save / resume (tests/test_gpu_checkpoint.py's flow) at 6 players with the return
    normalizer on: return_normalizer.json carries all N x 6 rolling returns, and the resumed
    context's next rollout matches an oracle trainer resumed from the same files"""
    import ctypes as C
    import os
    from bppo import checkpoint as K
    from test_gpu_checkpoint import _opt
    N, T, ctde, players = 48, 16, False, 6
    kw = dict(normalize_obs=True, normalize_returns=True, reward_shaping_coef=SHAPING)
    cfg, tr, ot = _pair(N, T, ctde, players, **kw)
    for _ in range(2):
        tr.train_update()
    mgr = K.CheckpointManager(str(tmp_path))
    meta = K.CheckpointMetadata.for_config(cfg, tr.global_step, 0.0)
    path = K.save_training_checkpoint(mgr, tr.ctx, tr.model.get_params(), meta)
    assert "return_normalizer.json" in os.listdir(path) and "normalizer.json" in os.listdir(path)
    rng_bytes = np.frombuffer(open(os.path.join(path, "rng_state.bin"), "rb").read(), np.uint8)
    saved = (tr.model.get_params(), _opt(tr.ctx), tr.ctx.obs_norm(), tr.ctx.ret_norm())
    mvc, rets = saved[3]
    assert rets.size == N * P and mvc[2] == 2 * N * T
    _seats_hold_returns(rets, N, players)                               # seats 4 and 5 too
    tr.close(); ot.close()

    cfg2, tr2, ot2 = _pair(N, T, ctde, players, **kw)
    K.resume_training_checkpoint(tr2.ctx, os.path.join(str(tmp_path), "checkpoints", "latest"))
    assert np.array_equal(tr2.model.get_params(), saved[0])
    for a, b in zip(_opt(tr2.ctx), saved[1]):
        assert np.array_equal(a, b)
    for a, b in zip(tr2.ctx.obs_norm(), saved[2]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for a, b in zip(tr2.ctx.ret_norm(), saved[3]):
        assert np.array_equal(a, b)
    assert tr2.ctx.rng_pos() == 0
    # the oracle resumed from the same files
    O.lib().or_trainer_set_params(ot2.h, np.ascontiguousarray(K.load_model(os.path.join(path, "model.mpk"))))
    m1, m2, st = saved[1]
    O.lib().or_trainer_set_adam(ot2.h, m1, m2, st, st.size)
    mean, m2n, cnt = saved[2]
    O.lib().or_trainer_set_norms(ot2.h, np.ascontiguousarray(mean).ctypes.data, np.ascontiguousarray(m2n).ctypes.data,
                                 float(cnt), np.ascontiguousarray(mvc).ctypes.data, np.ascontiguousarray(rets).ctypes.data)
    O.lib().or_trainer_set_rng(ot2.h, rng_bytes.view("<u4").copy(), 0)
    bppo.collect_rollouts(tr2.ctx); ot2.collect()
    _cmp_rollout(tr2, ot2, ctde, rew_rtol=2e-7)
    _cmp_norm_state(tr2, ot2, N)
    bppo.compute_gae(tr2.ctx); ot2.gae()
    np.testing.assert_allclose(tr2.buffer.advantages.reshape(-1), ot2.buffer("advantages"), rtol=1e-5, atol=1e-6)
    tr2.close(); ot2.close()
