"""Episode statistics on the device (bppo_set_episode_stats, csrc/episode_stats.hip): the
kernels against the host build of the same source, against the reference's logging restated in
tests/episode_ref.py on real rollouts, inside the pipelined loop, and switched off.

The rollout sizes (N, T) and the episode counts they give are pinned in
tests/test_episode_stats_ref.py (ROLLOUT_CASES), chosen there on the CPU oracle so that the
tail's selection (more than 100 episodes) and its take-all case (fewer) both run."""
import ctypes as C
import functools

import numpy as np
import pytest

import bppo
import bppo._lib as L
import episode_ref as R
from eval_ref import ENVS
from test_episode_stats_ref import ROLLOUT_CASES, SETS, rollout_cfg, run_block

pytestmark = pytest.mark.gpu


# ------------------------------------------------------ device against host ---
@pytest.mark.parametrize("tag,episodes,P", SETS, ids=[s[0] for s in SETS])
def test_kernels_equal_host_build(tag, episodes, P):
    host, dev = run_block(0, episodes, P), run_block(1, episodes, P)
    R.blocks_equal(dev, host, episodes, P, tag)
    R.check_block(dev[0], dev[1], episodes, P, tag)


def test_kernels_on_few_key_digits():
    """T N = 2^11 and 2^22: one and two digit passes"""
    for N, T, n in ((64, 32, 300), (2048, 2048, 3000)):
        eps = R.synthetic(n, 2, N, T, N + n, integer=False)
        R.blocks_equal(run_block(1, eps, 2, N=N, T=T), run_block(0, eps, 2, N=N, T=T), eps, 2, (N, T))


# ----------------------------------------------------------------- rollouts ---
def _trainer(env, **kw):
    cfg = rollout_cfg(env)
    return bppo.Trainer(cfg, params=bppo.orthogonal_init(cfg, seed=5), **kw)


def _episodes(ctx, P):
    """the last rollout's episodes with their outcomes, as tests/episode_ref.py takes them"""
    eps, outs = bppo.rollout_episodes(ctx), bppo.rollout_episode_outcomes(ctx)
    assert len(eps) == len(outs)
    return [dict(e, outcome=None if o is None else o[:P]) for e, o in zip(eps, outs)], outs


@functools.lru_cache(maxsize=None)
def rollout(env):
    k = ROLLOUT_CASES[env]
    tr = _trainer(env, episode_stats=True)
    info = bppo.collect_rollouts(tr.ctx)
    out = dict(info=info.episodes, block=bppo.episode_stats(tr.ctx, 0))
    out["episodes"], out["outcomes6"] = _episodes(tr.ctx, k["P"])
    out["actions"] = tr.ctx.buffer("actions", np.int32).reshape(k["T"], k["N"])
    out["seed_base"] = tr.ctx.struct.env_seed_base
    n = C.c_int32()
    raw = (L.Episode * 512)()
    tr.ctx._chk(L.lib().bppo_rollout_episodes(tr.ctx.h, raw, 512, C.byref(n)))
    out["pads"] = [raw[i].pad for i in range(min(n.value, 512))]
    tr.close()
    return out


@pytest.mark.parametrize("env", list(ROLLOUT_CASES))
def test_rollout_block_equals_restatement(env):
    r, k = rollout(env), ROLLOUT_CASES[env]
    stats, tail = r["block"]
    assert r["info"] == stats["episodes"] == stats["kept"] == len(r["episodes"]) == k["episodes"]
    R.check_block(stats, tail, r["episodes"], k["P"], env)
    assert len(tail) == min(100, k["episodes"])
    assert r["pads"] == [0] * k["episodes"]                   # the public record keeps pad = 0
    if k["P"] == 1:                                             # CartPole reports no outcome
        assert stats["with_outcome"] == 0 and all(o is None for o in r["outcomes6"])
    else:                                                       # every finished game does
        assert stats["with_outcome"] == k["episodes"] and all(t["placements"] is not None for t in tail)
        assert all(o[k["P"]:] == [0] * (6 - k["P"]) and min(o[:k["P"]]) >= 1 for o in r["outcomes6"])
    # the window over this one rollout: the reference's scalars (Liar's Dice pays fractions:
    # there its f32 running sums round and return_mean is held to the exact mean) and its deques
    w, ref_w = bppo.EpisodeWindow(k["P"]), R.Windows(k["P"])
    w.add(stats, tail)
    ref_w.push([dict(e, total_rewards=e["total_rewards"][:k["P"]]) for e in r["episodes"]])
    R.scalars_equal(w.scalars(), r["episodes"], k["P"], env)
    assert [float(x) for x in w.recent_returns] == [float(x) for x in ref_w.recent_returns]
    assert list(w.recent_outcomes) == list(ref_w.recent_outcomes)


@pytest.mark.parametrize("env", ["connect_four", "liars_dice", "skull"])
def test_rollout_outcomes_equal_replayed_games(env):
    """the device's actions through the oracle's envs: game_outcome read before the reset"""
    r, k = rollout(env), ROLLOUT_CASES[env]
    envs = [ENVS[env]((r["seed_base"] + i) & (2**64 - 1), k["P"]) for i in range(k["N"])]
    for e in envs:
        e.set_num_players(k["P"])
        e.reset()
    want = []
    for t in range(k["T"]):
        for i, e in enumerate(envs):
            _, d = e.step(int(r["actions"][t, i]))
            if d:
                oc = e.outcome()
                want.append((t, i, None if oc is None else [int(x) for x in oc[:k["P"]]]))
                e.reset()
    got = [(e["step"], e["env_index"], e["outcome"]) for e in r["episodes"]]
    assert got == want and len(want) == k["episodes"]
    assert len({tuple(o) for _, _, o in want}) > 1              # more than one result occurs


# ---------------------------------------------------------------- pipelined ---
def _metrics_equal(a, b):
    return list(a) == list(b) and np.array_equal(np.array(list(a.values()), np.float64),
                                                 np.array(list(b.values()), np.float64), equal_nan=True)


@pytest.mark.parametrize("env", ["connect_four", "cartpole"])
def test_pipelined_updates_report_every_rollout(env):
    """train_updates(3) with the statistics on: rollout k's block is the one a twin context's
    k-th train_step reports (whose episodes are read after each step), and parameters, RNG
    position and update metrics are those of a context with the statistics off"""
    P = ROLLOUT_CASES[env]["P"]
    on, twin, off = _trainer(env, episode_stats=True), _trainer(env, episode_stats=True), _trainer(env)
    m_on, _ = on.train_updates(3)
    m_off, _ = off.train_updates(3)
    blocks = [bppo.episode_stats(on.ctx, k) for k in range(3)]
    seen = []
    for k in range(3):
        twin.train_update()
        eps, _ = _episodes(twin.ctx, P)
        R.blocks_equal(blocks[k], bppo.episode_stats(twin.ctx, 0), eps, P, (env, k))
        R.check_block(blocks[k][0], blocks[k][1], eps, P, (env, k))
        assert m_on[k]["episodes"] == len(eps) > 0
        seen += eps
    assert blocks[0][1] != blocks[1][1]                        # three different rollouts
    assert on.episodes.scalars() == twin.episodes.scalars() == R.episode_scalars(seen, P)
    assert list(on.recent_returns) == list(twin.recent_returns) and len(on.recent_returns) == 100
    assert [float(x) for x in on.recent_returns] == [float(e["total_rewards"][0]) for e in seen[-100:]]
    with pytest.raises(bppo.BppoError) as ei:
        bppo.episode_stats(on.ctx, 3)
    assert ei.value.status == L.ERR_ARG and "rollout 3" in str(ei.value)
    # on == off
    assert all(_metrics_equal(a, b) for a, b in zip(m_on, m_off))
    assert on.ctx.rng_pos() == off.ctx.rng_pos() == twin.ctx.rng_pos()
    p_on, p_off = on.model.get_params(), off.model.get_params()
    assert np.array_equal(p_on.view(np.uint32), p_off.view(np.uint32))
    assert np.array_equal(p_on.view(np.uint32), twin.model.get_params().view(np.uint32))
    for t in (on, twin, off):
        t.close()


# ----------------------------------------------------------- off and errors ---
def test_off_by_default_and_errors():
    tr = _trainer("connect_four")
    assert tr.episodes is None
    info = bppo.collect_rollouts(tr.ctx)
    with pytest.raises(bppo.BppoError) as ei:
        bppo.episode_stats(tr.ctx, 0)
    assert ei.value.status == L.ERR_ARG and "off" in str(ei.value)
    # the outcomes do not need the statistics
    outs = bppo.rollout_episode_outcomes(tr.ctx)
    assert len(outs) == info.episodes == ROLLOUT_CASES["connect_four"]["episodes"] and all(o is not None for o in outs)
    bppo.set_episode_stats(tr.ctx, True)
    with pytest.raises(bppo.BppoError) as ei:                  # no rollout since
        bppo.episode_stats(tr.ctx, 0)
    assert ei.value.status == L.ERR_ARG and "no rollout" in str(ei.value)
    bppo.compute_gae(tr.ctx)
    bppo.ppo_update(tr.ctx, 1e-3, 0.01)
    bppo.collect_rollouts(tr.ctx)
    stats, tail = bppo.episode_stats(tr.ctx, 0)
    eps, _ = _episodes(tr.ctx, 2)
    R.check_block(stats, tail, eps, 2, "second rollout")
    for k in (-1, 1):
        with pytest.raises(bppo.BppoError) as ei:
            bppo.episode_stats(tr.ctx, k)
        assert ei.value.status == L.ERR_ARG
    # tail_cap below the tail: the first entries; *n_tail still the tail's length
    s, n = L.EpisodeStats(), C.c_int32()
    t3 = (L.EpisodeTail * 3)()
    tr.ctx._chk(L.lib().bppo_episode_stats_get(tr.ctx.h, 0, C.byref(s), t3, 3, C.byref(n)))
    assert n.value == len(tail) and [t3[i].step for i in range(3)] == [t["step"] for t in tail[:3]]
    bppo.set_episode_stats(tr.ctx, False)
    with pytest.raises(bppo.BppoError):
        bppo.episode_stats(tr.ctx, 0)
    tr.close()


# ------------------------------------------------------------ opponent pool ---
def test_opponent_pool_placements_agree():
    """envs below num_opponent_envs: the episode records' placements are the completions'"""
    k = ROLLOUT_CASES["connect_four"]
    N, n_opp, K = k["N"], k["N"] // 2, 3
    cfg = rollout_cfg("connect_four")
    tr = bppo.Trainer(cfg, params=bppo.orthogonal_init(cfg, seed=5), episode_stats=True)
    rng = np.random.default_rng(7)
    params = np.stack([bppo.orthogonal_init(cfg, seed=100 + j) for j in range(K)])
    lp = rng.integers(0, 2, n_opp).astype(np.int32)
    po = np.full((n_opp, 2), -1, np.int32)
    for e in range(n_opp):
        po[e, 1 - lp[e]] = rng.integers(0, K)
    tr.ctx.set_opponents(params, [None] * K, n_opp, lp, po, rng.integers(0, K, 1).astype(np.int32))
    bppo.collect_rollouts(tr.ctx)
    comps, dropped = tr.ctx.opponent_completions()
    eps, _ = _episodes(tr.ctx, 2)
    got = [(e["step"], e["env_index"], e["outcome"]) for e in eps if e["env_index"] < n_opp]
    assert dropped == 0 and len(comps) >= n_opp
    assert got == [(c["step"], c["env_index"], c["placements"]) for c in comps]
    stats, tail = bppo.episode_stats(tr.ctx, 0)
    R.check_block(stats, tail, eps, 2, "opponent pool")
    tr.close()
