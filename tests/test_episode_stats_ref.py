"""Episode statistics without a GPU: the host build of csrc/episode_stats.hip's source
(bppo_debug_episode_stats device 0) and bppo.EpisodeWindow against the reference's episode
logging restated in tests/episode_ref.py (main.rs:842-875, 1134-1217; env.rs:208-261).

The rollout tests of tests/test_gpu_episode_stats.py choose T per env from the CPU oracle
trainer's episode list for the seed (oracle_ffi.Trainer.episodes after one collect), so that
the tail's two regimes are both met: more than 100 finished episodes (a selection) and fewer
(every record is the tail).  ROLLOUT_CASES pins those counts; they are asserted here on the
oracle and there on the device."""
import ctypes as C

import numpy as np
import pytest

import bppo
import bppo._lib as L
import episode_ref as R
from bppo.episodes import pack_outcome

SETS = R.synthetic_sets()

# the rollout cases of tests/test_gpu_episode_stats.py: env -> preset, overrides, seated players,
# N, T and the finished episodes the oracle trainer counts for this seed and these parameters
# (orthogonal_init seed 5).  Other T tried: connect_four T = 32: 74; liars_dice T = 48: 76;
# skull T = 96: 69; cartpole T = 32: 155; cartpole48 T = 96: 131.
ROLLOUT_CASES = {
    "connect_four": dict(preset="connect_four", over={}, P=2, N=64, T=48, episodes=120),
    "liars_dice": dict(preset="liars_dice_ctde", over=dict(critic_hidden_size=64, critic_num_hidden=2), P=4, N=64,
                       T=64, episodes=127),
    "skull": dict(preset="skull", over=dict(player_count=3), P=3, N=64, T=128, episodes=88),
    "cartpole": dict(preset="cartpole", over={}, P=1, N=128, T=64, episodes=352),           # the fused 64 x 2 net
    "cartpole48": dict(preset="cartpole", over=dict(hidden_size=48), P=1, N=32, T=64, episodes=87),   # the GEMM path
}


def rollout_cfg(env, **kw):
    k = ROLLOUT_CASES[env]
    over = dict(num_envs=k["N"], num_steps=k["T"], hidden_size=64, num_hidden=2, normalize_obs=False,
                normalize_returns=False, reward_shaping_coef=0.0, num_epochs=2, num_minibatches=2, target_kl=None)
    over.update(k["over"])
    over.update(kw)
    return bppo.make_config(k["preset"], **over)


def oracle_episode_count(env):
    import oracle_ffi as O
    from bppo.host import shaping_schedule
    k, cfg = ROLLOUT_CASES[env], rollout_cfg(env)
    kind = {"connect_four": O.ENV_CONNECT_FOUR, "liars_dice": O.ENV_LIARS_DICE, "skull": O.ENV_SKULL}.get(
        env, O.ENV_CARTPOLE)
    ctde = cfg["network_type"] == "ctde"
    ocfg = O.train_cfg(env_kind=kind, num_envs=k["N"], num_steps=k["T"], seed=cfg["seed"], hidden=cfg["hidden_size"],
                       num_hidden=cfg["num_hidden"], ctde=ctde, relu=True,
                       critic_hidden=cfg["critic_hidden_size"] if ctde else 0,
                       critic_num_hidden=cfg["critic_num_hidden"] if ctde else 0, normalize_obs=False,
                       normalize_returns=False, gamma=cfg["gamma"], gae_lambda=cfg["gae_lambda"],
                       lr=bppo.schedule_get(cfg["learning_rate"], 0), ent_coef=bppo.schedule_get(cfg["entropy_coef"], 0),
                       reward_shaping=bppo.schedule_get(shaping_schedule(cfg), 0), num_epochs=2, num_minibatches=2,
                       clip=cfg["clip_epsilon"], value_coef=cfg["value_coef"], target_kl=None,
                       player_count=3 if env == "skull" else 0)
    ot = O.Trainer(ocfg, bppo.orthogonal_init(cfg, seed=5))
    ot.collect()
    n = len(ot.episodes())
    ot.close()
    return n


@pytest.mark.parametrize("env", list(ROLLOUT_CASES))
def test_rollout_cases_cover_both_tail_regimes(env):
    assert oracle_episode_count(env) == ROLLOUT_CASES[env]["episodes"]
    counts = [k["episodes"] for k in ROLLOUT_CASES.values()]
    assert min(counts) < 100 < max(counts) and all(k["N"] <= 128 and k["T"] <= 128 for k in ROLLOUT_CASES.values())


def run_block(device, episodes, P, N=R.SYN_N, T=R.SYN_T):
    words = [pack_outcome(e["outcome"]) for e in episodes]
    return bppo.debug_episode_stats(device, episodes, words, P, N, T)


def test_abi_struct_sizes():
    assert L.lib().bppo_episode_stats_size() == C.sizeof(L.EpisodeStats) == 200
    assert L.lib().bppo_episode_tail_size() == C.sizeof(L.EpisodeTail) == 64


@pytest.mark.parametrize("tag,episodes,P", SETS, ids=[s[0] for s in SETS])
def test_host_build_equals_restatement(tag, episodes, P):
    stats, tail = run_block(0, episodes, P)
    R.check_block(stats, tail, episodes, P, tag)
    assert len(tail) == min(100, len(episodes))


def test_sets_cover_the_cases():
    """what keeps the sets honest: counts around the tail's depth, a one-step batch, keys with
    three live digits, draws, the 1,1,3,3 tie, records without an outcome, 3 of 6 seats"""
    by = {t: (e, P) for t, e, P in SETS}
    assert {len(e) for t, (e, P) in by.items() if t.startswith("P")} == set(R.COUNTS)
    assert {P for t, (e, P) in by.items() if t.startswith("P")} == set(range(1, 7))
    one = by["one-step-3000"][0]
    assert len(one) == 3000 and len({e["step"] for e in one}) == 1
    keys = [e["step"] * R.SYN_N + e["env_index"] for e in by["spread-3000-frac"][0]]
    assert R.SYN_N * R.SYN_T == 2**23 and max(keys) >= 2**22 and len({k >> 12 for k in keys}) > 1000
    assert all(e["outcome"] == [1, 1, 1, 1] for e in by["all-draw"][0])
    assert all(e["outcome"] == [1, 1, 3, 3] for e in by["tie-1133"][0])
    assert all(e["outcome"] is None or len(e["outcome"]) == 3 for e in by["skull-3-of-6"][0])
    mixed = by["P4-n101"][0]
    assert any(e["outcome"] is None for e in mixed) and any(e["outcome"] is not None for e in mixed)
    # and the Swiss arithmetic on the two named outcomes (env.rs:236-242)
    s, _ = run_block(0, by["tie-1133"][0], 4)
    assert s["points2_sum"][:4] == [150 * 5, 150 * 5, 150 * 1, 150 * 1] and s["draws"] == 0
    s, _ = run_block(0, by["all-draw"][0], 4)
    assert s["points2_sum"][:4] == [150 * 3] * 4 and s["draws"] == s["with_outcome"] == 150


def test_debug_hook_rejects_bad_arguments_before_any_hip_call():
    eps = R.synthetic(4, 2, 8, 8, 1)
    ok = dict(device=1, episodes=eps, outcome_words=None, P=2, N=8, T=8)
    for bad in (dict(P=0), dict(P=7), dict(N=0), dict(T=0), dict(N=1), dict(T=1),
                dict(episodes=eps + [dict(eps[0])])):          # one (step, env_index) twice
        with pytest.raises(bppo.BppoError) as ei:
            bppo.debug_episode_stats(**dict(ok, **bad))
        assert ei.value.status == L.ERR_ARG, bad
    s, nt = L.EpisodeStats(), C.c_int32()
    tail = (L.EpisodeTail * 100)()
    assert L.lib().bppo_debug_episode_stats(1, 1, None, None, 2, 8, 8, C.byref(s), tail, C.byref(nt)) == L.ERR_ARG
    assert L.lib().bppo_debug_episode_stats(1, 0, None, None, 2, 8, 8, None, tail, C.byref(nt)) == L.ERR_ARG
    assert L.lib().bppo_episode_stats_get(None, 0, None, None, 0, None) == L.ERR_ARG
    assert L.lib().bppo_set_episode_stats(None, 1) == L.ERR_ARG
    assert L.lib().bppo_rollout_episode_outcomes(None, None, None, 0, None) == L.ERR_ARG


# ------------------------------------------------------------- EpisodeWindow ---
def window_blocks(P, seed, k=4, frac=False, outcome="mixed"):
    """k rollouts' episodes: whole-number returns (frac: multiples of 1/2), so the reference's
    sequential f32 sums are exact and every scalar must match bit for bit"""
    blocks = []
    for i in range(k):
        eps = R.synthetic((150, 37, 0, 120, 260)[i % 5], P, 64, 128, seed + i, outcome=outcome)
        if frac:
            for e in eps:
                e["total_rewards"] = [np.float32(x * 0.5) for x in e["total_rewards"]]
        blocks.append(eps)
    return blocks


@pytest.mark.parametrize("outcome", ["all", "mixed"])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 6])
def test_window_merges_rollouts_into_the_reference_scalars(P, outcome):
    """outcome "all": every finished game reports its game_outcome, as every game of the
    device's envs does; the three deques are then the reference's.  "mixed" (a fifth of the
    episodes without one): the scalars and the return deques are still the reference's;
    recent_outcomes is fed from each rollout's last 100 EPISODES, so it holds the outcomes among
    those, where the reference's own deque would reach further back for its 100 outcomes."""
    blocks = window_blocks(P, 1000 * P, k=5, frac=P % 2 == 0, outcome=outcome)
    w, ref_w, seen = bppo.EpisodeWindow(P), R.Windows(P), []
    for eps in blocks:
        w.add(*run_block(0, eps, P, N=64, T=128))
        if outcome == "all":
            ref_w.push(R.rollout_order(eps))
        else:
            ref_w.push([dict(e, outcome=e["outcome"] if i >= len(eps) - 100 else None)
                        for i, e in enumerate(R.rollout_order(eps))])
        seen += R.rollout_order(eps)
        want = R.episode_scalars(seen, P)
        got = w.scalars()
        assert list(got) == list(want) and got == want, (got, want)
        assert [float(x) for x in w.recent_returns] == [float(x) for x in ref_w.recent_returns]
        for p in range(P):
            assert [float(x) for x in w.recent_returns_per_player[p]] == \
                   [float(x) for x in ref_w.recent_returns_per_player[p]]
        assert list(w.recent_outcomes) == list(ref_w.recent_outcomes)
    assert len(w.recent_returns) == 100 and ("episode/draw_rate" in got) == (P > 1)
    # clear(): a new log interval; the rolling windows stay
    w.clear()
    assert w.scalars() == {} and len(w.recent_returns) == 100
    w.add(*run_block(0, blocks[0], P, N=64, T=128))
    assert w.scalars() == R.episode_scalars(R.rollout_order(blocks[0]), P)


def test_window_merge_of_windows_is_exact():
    """two ranks' windows merged == one window fed both ranks' rollouts"""
    P = 4
    blocks = window_blocks(P, 77, k=4)
    a, b, both = bppo.EpisodeWindow(P), bppo.EpisodeWindow(P), bppo.EpisodeWindow(P)
    for i, eps in enumerate(blocks):
        blk = run_block(0, eps, P, N=64, T=128)
        (a if i % 2 == 0 else b).add(*blk)
        both.add(*blk)
    a.merge(b)
    assert a.scalars() == both.scalars() == R.episode_scalars([e for eps in blocks for e in eps], P)
    assert a.episodes == sum(len(e) for e in blocks)


def test_empty_window():
    w = bppo.EpisodeWindow(2)
    assert w.scalars() == {}
    w.add(*run_block(0, [], 2))
    assert w.scalars() == {} and len(w.recent_returns) == 0
    # a window whose games reported no outcome: compute_avg_points' early return
    eps = R.synthetic(5, 2, 64, 128, 3, outcome="none")
    w.add(*run_block(0, eps, 2, N=64, T=128))
    got = w.scalars()
    assert got == R.episode_scalars(R.rollout_order(eps), 2) and got["episode/draw_rate"] == 0.0
    assert "episode/avg_points_p0" not in got and got["episode/games_completed"] == 5.0


def test_return_mean_is_f32_of_the_f64_mean():
    """where the reference's f32 running sum rounds, the window reports the better value"""
    eps = R.synthetic(260, 2, 64, 128, 5, integer=False)
    w = bppo.EpisodeWindow(2)
    w.add(*run_block(0, eps, 2, N=64, T=128))
    got, want = w.scalars(), R.episode_scalars(R.rollout_order(eps), 2)
    import math
    for p in range(2):
        xs = [float(np.float32(e["total_rewards"][p])) for e in eps]
        exact = math.fsum(xs) / len(xs)
        k = f"episode/return_mean_p{p}"
        assert got[k] == float(np.float32(exact))
        assert abs(want[k] - exact) <= 260 * 2.0**-24 * math.fsum(abs(x) for x in xs) / 260   # the reference's own error
    for k in got:
        if "return_mean" not in k:
            assert got[k] == want[k], k
