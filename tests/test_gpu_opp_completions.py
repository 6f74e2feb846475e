"""Finished opponent-pool games leave the device: bppo_opponents_completions /
bppo_opponents_results (ppo.rs:505-521, 871-917; opponent_pool.rs:578-616) and PoolTrainer.

Per env kind one T-step rollout is compared with T one-step rollouts of a second context
(same seed, models and seats).  The one-step path returns to the host after every step, so
the seats a game was played under are those bppo_opponents_get_envs showed before the
call; the placements are checked by replaying the device's actions through the oracle's
envs (tests/eval_ref.py), whose game_outcome is read before the reset.

T per env kind was chosen on the CPU from the oracle trainer's episode list for this seed
(oracle_ffi.Trainer.episodes after one T-step collect with the same models and seats):
    connect_four  T = 56:  112 finished opponent games, 46 envs finish twice or more
    liars_dice    T = 80:  120 finished opponent games, 48 envs finish twice or more
    skull (P = 3) T = 176: 108 finished opponent games, 47 envs finish twice or more
each at least 2 * n_opp = 96 games; an env that finishes twice plays its second game on
seats the device drew.  The tests assert those counts on the device's results."""
import ctypes as C
import functools

import numpy as np
import pytest

import bppo
import bppo._lib as L
import oracle_ffi as O
from bppo.host import shaping_schedule
from eval_ref import ENVS

pytestmark = pytest.mark.gpu

N, N_OPP, K = 64, 48, 3
KINDS = {
    "connect_four": dict(preset="connect_four", kind=O.ENV_CONNECT_FOUR, P=2, T=56, games=112, twice=46, over={}),
    "liars_dice": dict(preset="liars_dice_ctde", kind=O.ENV_LIARS_DICE, P=4, T=80, games=120, twice=48,
                       over=dict(critic_hidden_size=64, critic_num_hidden=2)),
    "skull": dict(preset="skull", kind=O.ENV_SKULL, P=3, T=176, games=108, twice=47, over=dict(player_count=3)),
}


def make_cfg(env, T, **kw):
    k = KINDS[env]
    over = dict(num_envs=N, num_steps=T, hidden_size=64, num_hidden=2, normalize_obs=False, normalize_returns=False,
                reward_shaping_coef=0.0, num_epochs=2, num_minibatches=2, target_kl=None)
    over.update(k["over"])
    over.update(kw)
    return bppo.make_config(k["preset"], **over)


def models_and_seats(env, cfg):
    """K random-initialised opponents and a seat table (as tests/test_gpu_skull.py draws it)"""
    P = KINDS[env]["P"]
    rng = np.random.default_rng(7)
    params = np.stack([bppo.orthogonal_init(cfg, seed=100 + k) for k in range(K)])
    lp = rng.integers(0, P, N_OPP).astype(np.int32)
    po = np.full((N_OPP, P), -1, np.int32)
    for e in range(N_OPP):
        for p in range(P):
            if p != lp[e]:
                po[e, p] = rng.integers(0, K)
    co = rng.integers(0, K, P - 1).astype(np.int32)
    return params, lp, po, co


def oracle_trainer(env, T):
    """the CPU oracle's trainer on the same configuration (how T was chosen; see the module docstring)"""
    k = KINDS[env]
    cfg = make_cfg(env, T)
    ctde = cfg["network_type"] == "ctde"
    ocfg = O.train_cfg(env_kind=k["kind"], num_envs=N, num_steps=T, seed=cfg["seed"], hidden=cfg["hidden_size"],
                       num_hidden=cfg["num_hidden"], ctde=ctde, relu=True,
                       critic_hidden=cfg["critic_hidden_size"] if ctde else 0,
                       critic_num_hidden=cfg["critic_num_hidden"] if ctde else 0, normalize_obs=False,
                       normalize_returns=False, gamma=cfg["gamma"], gae_lambda=cfg["gae_lambda"],
                       lr=bppo.schedule_get(cfg["learning_rate"], 0), ent_coef=bppo.schedule_get(cfg["entropy_coef"], 0),
                       reward_shaping=bppo.schedule_get(shaping_schedule(cfg), 0), num_epochs=cfg["num_epochs"],
                       num_minibatches=cfg["num_minibatches"], clip=cfg["clip_epsilon"], value_coef=cfg["value_coef"],
                       target_kl=cfg["target_kl"], player_count=k["P"] if env == "skull" else 0)
    ot = O.Trainer(ocfg, bppo.orthogonal_init(cfg, seed=5))
    params, lp, po, co = models_and_seats(env, cfg)
    ot.set_opponents(params, [None] * K, N_OPP, lp, po.reshape(-1), co)
    return ot


def replay_envs(env, seed_base):
    """the oracle's per-env structs as VecEnv::new leaves them: E::new(seed_base + i), the seated
    player count, reset()"""
    P = KINDS[env]["P"]
    envs = [ENVS[env]((seed_base + i) & (2**64 - 1), P) for i in range(N)]
    for e in envs:
        e.set_num_players(P)
        e.reset()
    return envs


def replay_step(envs, actions):
    """VecEnv::step with the given actions -> (dones [N], {env: game_outcome or None}); the
    outcome is read before the auto-reset (env.rs:442-450)"""
    dones, outcomes = np.zeros(N, bool), {}
    for i, e in enumerate(envs):
        _, d = e.step(int(actions[i]))
        if d:
            dones[i] = True
            outcomes[i] = e.outcome()
            e.reset()
    return dones, outcomes


def _trainer(env, T, **kw):
    cfg = make_cfg(env, T, **kw)
    tr = bppo.Trainer(cfg, params=bppo.orthogonal_init(cfg, seed=5))
    params, lp, po, co = models_and_seats(env, cfg)
    tr.ctx.set_opponents(params, [None] * K, N_OPP, lp, po, co)
    return tr, co


def _queue_sums(comps):
    """queue_game_result applied to completions, per device model slot"""
    wins, games, swiss = np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros(K, np.int64)
    for c in comps:
        pl, lp = c["placements"], c["learner_position"]
        for seat, m in enumerate(c["position_to_opponent"]):
            if seat == lp:
                continue
            games[m] += 1
            swiss[m] += len(pl) - pl[lp]
            wins[m] += pl[lp] < pl[seat]
    return wins, games, swiss


@functools.lru_cache(maxsize=None)
def run(env):
    """T one-step rollouts and one T-step rollout of two contexts with the same seed"""
    T, P = KINDS[env]["T"], KINDS[env]["P"]
    one, co = _trainer(env, 1)
    envs = replay_envs(env, one.ctx.struct.env_seed_base)
    out = dict(comps=[], actions=[], players=[], seats_before=[], seats_after=[], episodes=[], outcomes=[],
               dones=[], results=[], dropped=[], cur=co)
    for t in range(T):
        out["seats_before"].append(tuple(a.copy() for a in one.ctx.opponent_envs()))
        bppo.collect_rollouts(one.ctx)
        comps, dropped = one.ctx.opponent_completions()
        out["comps"].append(comps)
        out["dropped"].append(dropped)
        out["results"].append(one.ctx.opponent_results())
        out["episodes"].append(bppo.rollout_episodes(one.ctx))
        out["seats_after"].append(tuple(a.copy() for a in one.ctx.opponent_envs()))
        acts = one.ctx.buffer("actions", np.int32)
        out["actions"].append(acts)
        out["players"].append(one.ctx.buffer("players", np.int32))
        out["dones"].append(one.ctx.buffer("dones") != 0)
        d, oc = replay_step(envs, acts)
        out["replay_dones"] = out.get("replay_dones", []) + [d]
        out["outcomes"].append(oc)
    one.close()
    multi, _ = _trainer(env, T)
    bppo.collect_rollouts(multi.ctx)
    out["multi"] = dict(comps=multi.ctx.opponent_completions(), results=multi.ctx.opponent_results(),
                        actions=multi.ctx.buffer("actions", np.int32).reshape(T, N),
                        players=multi.ctx.buffer("players", np.int32).reshape(T, N),
                        episodes=bppo.rollout_episodes(multi.ctx), seats_after=multi.ctx.opponent_envs())
    # capacity 1: the first record only; the counts and the sums are unchanged
    rec, n, dr = (L.OppCompletion * 1)(), C.c_int32(-1), C.c_int32(-1)
    multi.ctx._chk(L.lib().bppo_opponents_completions(multi.ctx.h, rec, 1, C.byref(n), C.byref(dr)))
    out["cap1"] = dict(n=n.value, dropped=dr.value, env_index=rec[0].env_index, step=rec[0].step,
                       placement=list(rec[0].placement), results=multi.ctx.opponent_results(),
                       again=multi.ctx.opponent_completions())
    multi.close()
    return out


ENV_IDS = list(KINDS)


def test_abi_struct_size():
    assert L.lib().bppo_opp_completion_size() == C.sizeof(L.OppCompletion) == 64


@pytest.mark.parametrize("env", ENV_IDS)
def test_one_step_seats(env):
    """every completion of call k carries step 0 and the seats read before call k; the
    completions are the finished envs < n_opp in ascending order; unfinished envs keep
    their seats and finished ones are reseated with the current opponents"""
    r, P = run(env), KINDS[env]["P"]
    n_games = 0
    for t, comps in enumerate(r["comps"]):
        lp0, po0 = r["seats_before"][t]
        lp1, po1 = r["seats_after"][t]
        fin = [e["env_index"] for e in r["episodes"][t] if e["env_index"] < N_OPP]
        assert [c["env_index"] for c in comps] == sorted(fin), t
        assert sorted(fin) == [int(i) for i in np.flatnonzero(r["dones"][t][:N_OPP])], t
        assert r["dropped"][t] == 0
        for c in comps:
            e = c["env_index"]
            assert c["step"] == 0 and c["learner_position"] == lp0[e], (t, e)
            assert c["position_to_opponent"] == [int(x) for x in po0[e]], (t, e)
            assert len(c["placements"]) == P and c["position_to_opponent"][c["learner_position"]] == -1
        for e in range(N_OPP):
            if e in fin:     # sample_all_slots + shuffle_positions: the current opponents on the other seats
                assert po1[e][lp1[e]] == -1
                assert sorted(int(x) for i, x in enumerate(po1[e]) if i != lp1[e]) == sorted(int(x) for x in r["cur"])
            else:
                assert lp1[e] == lp0[e] and np.array_equal(po1[e], po0[e]), (t, e)
        if t + 1 < len(r["comps"]):
            nlp, npo = r["seats_before"][t + 1]
            assert np.array_equal(nlp, lp1) and np.array_equal(npo, po1)
        n_games += len(comps)
    assert n_games == KINDS[env]["games"] >= 2 * N_OPP


@pytest.mark.parametrize("env", ENV_IDS)
def test_placements_match_replayed_outcomes(env):
    """the device's actions replayed through the oracle's envs: each finished game's
    game_outcome, read before the reset, is the record's placements"""
    r, P = run(env), KINDS[env]["P"]
    n, not_reward_rank = 0, 0
    for t, comps in enumerate(r["comps"]):
        assert np.array_equal(r["replay_dones"][t], r["dones"][t]), t
        by_env = {c["env_index"]: c for c in comps}
        for e, oc in r["outcomes"][t].items():
            if e >= N_OPP:
                continue
            if oc is None:
                assert e not in by_env, (t, e)
                continue
            assert by_env[e]["placements"] == [int(x) for x in oc[:P]], (t, e)
            n += 1
        assert set(by_env) <= set(r["outcomes"][t]), t
    assert n == KINDS[env]["games"]


@pytest.mark.parametrize("env", ENV_IDS)
def test_multi_step_equals_one_step_rollouts(env):
    r, T = run(env), KINDS[env]["T"]
    m = r["multi"]
    # the rollout draws nothing between steps: T one-step rollouts are the T-step rollout
    for t in range(T):
        assert np.array_equal(m["actions"][t], r["actions"][t]), t
        assert np.array_equal(m["players"][t], r["players"][t]), t
    comps, dropped = m["comps"]
    want = [dict(c, step=t) for t in range(T) for c in r["comps"][t]]
    assert dropped == 0 and comps == want
    assert np.array_equal(m["seats_after"][0], r["seats_after"][-1][0])
    assert np.array_equal(m["seats_after"][1], r["seats_after"][-1][1])
    # what keeps this honest: enough games, games on device-drawn seats, wins and losses
    assert len(comps) == KINDS[env]["games"] >= 2 * N_OPP
    per_env = np.bincount([c["env_index"] for c in comps], minlength=N_OPP)
    assert int((per_env >= 2).sum()) == KINDS[env]["twice"] >= 1
    lplace = [c["placements"][c["learner_position"]] for c in comps]
    assert min(lplace) == 1 and max(lplace) > 1
    first = {}
    for c in comps:                       # a later game of an env sits on seats a reshuffle drew
        first.setdefault(c["env_index"], c)
    assert any(c["position_to_opponent"] != first[c["env_index"]]["position_to_opponent"] for c in comps)
    # and the episode list names the same finished games
    eps = [(e["step"], e["env_index"]) for e in m["episodes"] if e["env_index"] < N_OPP]
    assert eps == [(c["step"], c["env_index"]) for c in comps]


@pytest.mark.parametrize("env", ENV_IDS)
def test_results_are_queue_game_result_sums(env):
    r = run(env)
    comps, _ = r["multi"]["comps"]
    wins, games, swiss = r["multi"]["results"]
    w, g, s = _queue_sums(comps)
    assert np.array_equal(wins, w) and np.array_equal(games, g) and np.array_equal(swiss, s)
    assert games.sum() == len(comps) * (KINDS[env]["P"] - 1) and 0 < wins.sum() < games.sum()
    for t, c1 in enumerate(r["comps"]):     # and per one-step rollout
        w, g, s = _queue_sums(c1)
        assert all(np.array_equal(a, b) for a, b in zip(r["results"][t], (w, g, s))), t
    # the same sums through the pool: device sums == game by game
    a = bppo.OpponentPool(KINDS[env]["P"], 0.1, 1.0, 1)
    b = bppo.OpponentPool(KINDS[env]["P"], 0.1, 1.0, 1)
    for p in (a, b):
        for k in range(K):
            p.add_checkpoint(f"step_{k}", k, np.zeros(1, np.float32))
    for c in comps:
        a.queue_game_result(c["placements"], c["learner_position"], c["position_to_opponent"])
    b.queue_results(wins, games, swiss, list(range(K)))
    assert a.pending_rotation_stats == b.pending_rotation_stats


@pytest.mark.parametrize("env", ENV_IDS)
def test_capacity_one_returns_the_first_record(env):
    r, P = run(env), KINDS[env]["P"]
    comps, _ = r["multi"]["comps"]
    c1 = r["cap1"]
    assert c1["n"] == len(comps) and c1["dropped"] == 0      # *n counts every recorded game, not only those copied
    assert (c1["env_index"], c1["step"]) == (comps[0]["env_index"], comps[0]["step"])
    assert c1["placement"] == comps[0]["placements"] + [0] * (6 - P)
    assert all(np.array_equal(a, b) for a, b in zip(c1["results"], r["multi"]["results"]))
    assert c1["again"] == r["multi"]["comps"]                # reading does not consume


def test_lifetime_train_steps_and_opponents_set():
    """after bppo_train_steps(n = 2) the completions and the episodes describe the same
    (the second) rollout; bppo_opponents_set empties both"""
    env = "connect_four"
    T = KINDS[env]["T"]
    tr, co = _trainer(env, T)
    tr.train_updates(2)
    comps, dropped = tr.ctx.opponent_completions()
    eps = [(e["step"], e["env_index"]) for e in bppo.rollout_episodes(tr.ctx) if e["env_index"] < N_OPP]
    assert dropped == 0 and len(comps) >= N_OPP
    assert eps == [(c["step"], c["env_index"]) for c in comps]
    w, g, s = _queue_sums(comps)
    assert all(np.array_equal(a, b) for a, b in zip(tr.ctx.opponent_results(), (w, g, s)))
    # one train_step more replaces them (not appends)
    bppo.train_step(tr.ctx, 1e-3, 0.01)
    comps2, _ = tr.ctx.opponent_completions()
    eps2 = [(e["step"], e["env_index"]) for e in bppo.rollout_episodes(tr.ctx) if e["env_index"] < N_OPP]
    assert eps2 == [(c["step"], c["env_index"]) for c in comps2] and comps2 != comps
    lp, po = tr.ctx.opponent_envs()
    params, _, _, _ = models_and_seats(env, tr.cfg)
    tr.ctx.set_opponents(params, [None] * K, N_OPP, lp, po, co)
    assert tr.ctx.opponent_completions() == ([], 0)
    assert bppo.rollout_episodes(tr.ctx) == []
    assert all(int(a.sum()) == 0 for a in tr.ctx.opponent_results())
    tr.close()


def test_no_opponents_is_an_argument_error():
    tr = bppo.Trainer(make_cfg("connect_four", 4))
    for call in (tr.ctx.opponent_completions, tr.ctx.opponent_results):
        with pytest.raises(bppo.BppoError) as ei:
            call()
        assert ei.value.status == L.ERR_ARG and "no opponents set" in str(ei.value)
    tr.close()


def _pool_run(seed):
    cfg = make_cfg("connect_four", 16)
    pool = bppo.OpponentPool(2, 0.1, 1.0, seed)
    for k in range(4):
        pool.add_checkpoint(f"step_{(k + 1) * 1000:08d}", (k + 1) * 1000, bppo.orthogonal_init(cfg, seed=200 + k))
    pt = bppo.PoolTrainer(cfg, pool, N_OPP, params=bppo.orthogonal_init(cfg, seed=5))
    played, slots, perf = [], [], []
    for _ in range(6):
        m = pt.step()
        played.append(sum(s.games_played for s in pool.available))
        slots.append(pt.device_slots())
        perf.append(m["pool_performance"])
        assert all(0.0 <= s.win_rate <= 1.0 for s in pool.available)
        assert 1 <= len(pt.device_slots()) <= 15 and m["opponent_games"] >= 0
        assert set(pool.current_opponents) <= set(pt.device_slots())
    stats = [(s.checkpoint_name, s.win_rate, s.avg_swiss_points, s.games_played) for s in pool.available]
    hist = [list(h) for h in pt.history]
    pt.close()
    return played, stats, hist, slots, perf


def test_pool_trainer_smoke():
    played, stats, hist, slots, perf = _pool_run(3)
    assert all(b >= a for a, b in zip(played, played[1:])) and played[-1] > played[0] >= 0     # games_played grows
    assert any(s[1] != 0.5 for s in stats) and all(p is None or 0.0 <= p <= 1.0 for p in perf)
    assert len(hist) == 6 and all(len(h) == 1 for h in hist)
    again = _pool_run(3)
    assert again[1] == stats and again[2] == hist and again[3] == slots
