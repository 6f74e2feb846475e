"""The reference's episode/* scalars and last-100 windows from the device's per-rollout
episode statistics (bppo_set_episode_stats, csrc/episode_stats.hip).

    main.rs:842-875    recent_returns / recent_returns_per_player / recent_outcomes
    main.rs:1134-1217  episode/length_*, episode/count, episode/return_*_p{p},
                       episode/avg_points_p{p}, episode/draw_rate, episode/games_completed
    env.rs:208-261     compute_avg_points

A rollout leaves a mergeable block of sums, counts and extremes and its last 100 episodes;
EpisodeWindow merges the blocks of a log interval.  No episode record crosses PCIe, so this
works inside the pipelined loop (Trainer.train_updates).
"""
import ctypes as C
from collections import deque

import numpy as np

from . import _lib as L

TAIL = L.EPISODE_TAIL
_F32 = np.float32


def set_episode_stats(ctx, enable=True):
    """bppo_set_episode_stats: every rollout from now on leaves its statistics and tail"""
    ctx._chk(L.lib().bppo_set_episode_stats(ctx.h, 1 if enable else 0))


def stats_dict(s):
    """bppo_episode_stats -> dict of Python ints / floats and numpy float32 extremes"""
    return dict(episodes=int(s.episodes), kept=int(s.kept), length_sum=int(s.length_sum),
                length_min=int(s.length_min), length_max=int(s.length_max), with_outcome=int(s.with_outcome),
                draws=int(s.draws), return_sum=[float(x) for x in s.return_sum],
                return_min=[_F32(x) for x in s.return_min], return_max=[_F32(x) for x in s.return_max],
                outcome_games=[int(x) for x in s.outcome_games], points2_sum=[int(x) for x in s.points2_sum])


_TAIL_DT = np.dtype([("total_reward", np.float32, L.MAX_PLAYERS), ("placement", np.int32, L.MAX_PLAYERS),
                     ("length", np.int32), ("env_index", np.int32), ("step", np.int32), ("has_outcome", np.int32)])


def tail_list(tail, n):
    """bppo_episode_tail [n] -> dicts; placements is None where the env reported no outcome
    (read through one numpy view of the array: a field-by-field ctypes walk of 100 records cost
    more than the rollout's kernels)"""
    a = np.frombuffer(tail, dtype=_TAIL_DT, count=n)
    tr, pl, has = a["total_reward"], a["placement"].tolist(), a["has_outcome"].tolist()
    ln, env, step = a["length"].tolist(), a["env_index"].tolist(), a["step"].tolist()
    return [dict(total_rewards=list(tr[i]), length=ln[i], env_index=env[i], step=step[i],
                 placements=pl[i] if has[i] else None) for i in range(n)]


def episode_stats(ctx, k=0):
    """bppo_episode_stats_get: rollout k of the last hot-path call -> (stats dict, tail list,
    oldest first in the reference's push order)"""
    s, n = L.EpisodeStats(), C.c_int32()
    tail = (L.EpisodeTail * TAIL)()
    ctx._chk(L.lib().bppo_episode_stats_get(ctx.h, k, C.byref(s), tail, TAIL, C.byref(n)))
    return stats_dict(s), tail_list(tail, min(n.value, TAIL))


def rollout_episode_outcomes(ctx):
    """game_outcome of the last rollout's episodes in rollout_episodes' order: the placements
    [6] per seat (0 beyond the seated players), None where the env reported none"""
    n = C.c_int32()
    ctx._chk(L.lib().bppo_rollout_episode_outcomes(ctx.h, None, None, 0, C.byref(n)))
    cap = n.value
    if cap == 0:
        return []
    pl, has = np.zeros((cap, L.MAX_PLAYERS), np.int32), np.zeros(cap, np.int32)
    ctx._chk(L.lib().bppo_rollout_episode_outcomes(ctx.h, pl.ctypes.data, has.ctypes.data, cap, C.byref(n)))
    return [[int(x) for x in pl[i]] if has[i] else None for i in range(min(n.value, cap))]


def debug_episode_stats(device, episodes, outcome_words, P, N, T):
    """bppo_debug_episode_stats on episode dicts (total_rewards, length, env_index, step) ->
    (stats dict, tail list); device 0 = the host build, 1 = the kernels"""
    n = len(episodes)
    eps = (L.Episode * max(n, 1))()
    for i, e in enumerate(episodes):
        for p, x in enumerate(e["total_rewards"]):
            eps[i].total_reward[p] = x
        eps[i].length, eps[i].env_index, eps[i].step = e["length"], e["env_index"], e["step"]
    words = None if outcome_words is None else np.ascontiguousarray(outcome_words, np.int32)
    s, nt = L.EpisodeStats(), C.c_int32()
    tail = (L.EpisodeTail * TAIL)()
    st = L.lib().bppo_debug_episode_stats(device, n, eps, None if words is None else words.ctypes.data, P, N, T,
                                          C.byref(s), tail, C.byref(nt))
    if st != L.OK:
        raise L.BppoError(st, "bppo_debug_episode_stats")
    return stats_dict(s), tail_list(tail, nt.value)


def pack_outcome(placements):
    """the episode record's outcome word (csrc/bppo_wide.h opp_pack_outcome); None = no outcome"""
    if placements is None:
        return 0
    w = 1 << 24
    for p, x in enumerate(placements):
        w |= (int(x) & 15) << (4 * p)
    return w


class EpisodeWindow:
    """The finished episodes since the last clear() as the reference logs them, and the
    rolling 100-episode windows.

    add(stats, tail) takes one rollout's block; merge(other) another window's (W > 1 ranks,
    or several windows): sums and counts add, extremes combine, so the merge is exact and
    needs no collective.  The deques take the tails oldest first: after a rollout they hold
    what main.rs:842-875 keeps.  recent_outcomes takes the outcomes among each rollout's last
    100 episodes: the reference's deque whenever every finished game reports an outcome, as
    every game of Connect Four, Liar's Dice and Skull does; a rollout in which some did not
    would leave the reference's deque reaching further back than its last 100 episodes.

    scalars() uses the reference's names and arithmetic.  Every value equals the
    reference's bit for bit wherever the reference's own sums are exact; return_mean_p{p}
    is f32(f64 sum / n), where the reference adds the returns one by one in f32: the two
    agree exactly for integer returns below 2^24 in sum and otherwise to f32 rounding of
    the reference's running sum."""

    def __init__(self, num_players):
        self.num_players = int(num_players)
        self.recent_returns = deque(maxlen=TAIL)
        self.recent_returns_per_player = [deque(maxlen=TAIL) for _ in range(self.num_players)]
        self.recent_outcomes = deque(maxlen=TAIL)
        self.clear()

    def clear(self):
        """the log interval's statistics start over (episodes_since_log.clear()); the
        rolling windows stay"""
        P = self.num_players
        self.episodes = self.kept = self.length_sum = self.with_outcome = self.draws = 0
        self.length_min, self.length_max = 2**31 - 1, 0
        self.return_sum = [0.0] * P
        self.return_min = [_F32(np.inf)] * P
        self.return_max = [_F32(-np.inf)] * P
        self.outcome_games = [0] * P
        self.points2_sum = [0] * P

    def _merge_stats(self, s):
        self.episodes += s["episodes"]
        self.kept += s["kept"]
        self.length_sum += s["length_sum"]
        self.length_min = min(self.length_min, s["length_min"])
        self.length_max = max(self.length_max, s["length_max"])
        self.with_outcome += s["with_outcome"]
        self.draws += s["draws"]
        for p in range(self.num_players):
            self.return_sum[p] += s["return_sum"][p]
            self.return_min[p] = min(self.return_min[p], _F32(s["return_min"][p]))
            self.return_max[p] = max(self.return_max[p], _F32(s["return_max"][p]))
            self.outcome_games[p] += s["outcome_games"][p]
            self.points2_sum[p] += s["points2_sum"][p]

    def add(self, stats, tail=()):
        """one rollout: its bppo_episode_stats (episode_stats' dict) and its tail"""
        self._merge_stats(stats)
        for ep in tail:
            self.recent_returns.append(ep["total_rewards"][0])                 # main.rs:844-853
            for p in range(self.num_players):
                self.recent_returns_per_player[p].append(ep["total_rewards"][p])
            if ep["placements"] is not None:
                self.recent_outcomes.append(list(ep["placements"][:self.num_players]))

    def merge(self, other):
        """another window's interval into this one; its rolling windows are appended after
        this one's (ranks have no common episode order)"""
        assert other.num_players == self.num_players
        self._merge_stats(dict(episodes=other.episodes, kept=other.kept, length_sum=other.length_sum,
                               length_min=other.length_min, length_max=other.length_max,
                               with_outcome=other.with_outcome, draws=other.draws, return_sum=other.return_sum,
                               return_min=other.return_min, return_max=other.return_max,
                               outcome_games=other.outcome_games, points2_sum=other.points2_sum))
        self.recent_returns.extend(other.recent_returns)
        for p in range(self.num_players):
            self.recent_returns_per_player[p].extend(other.recent_returns_per_player[p])
        self.recent_outcomes.extend(other.recent_outcomes)

    def scalars(self):
        """{name: value} of main.rs:1134-1217 for the interval; {} when no episode finished"""
        n = self.kept
        if n == 0:
            return {}
        out = {"episode/length_mean": float(_F32(self.length_sum) / _F32(n)),
               "episode/length_max": float(_F32(self.length_max)),
               "episode/length_min": float(_F32(self.length_min)),
               "episode/count": float(_F32(n))}
        for p in range(self.num_players):
            out[f"episode/return_mean_p{p}"] = float(_F32(self.return_sum[p] / n))
            out[f"episode/return_max_p{p}"] = float(self.return_max[p])
            out[f"episode/return_min_p{p}"] = float(self.return_min[p])
        if self.num_players > 1:
            for p in range(self.num_players):
                if self.outcome_games[p] > 0:
                    out[f"episode/avg_points_p{p}"] = float(_F32((self.points2_sum[p] / 2.0) / self.outcome_games[p]))
            # compute_avg_points returns 0.0 for no outcomes (env.rs:212-214)
            out["episode/draw_rate"] = float(_F32(self.draws) / _F32(self.with_outcome)) if self.with_outcome else 0.0
            out["episode/games_completed"] = float(_F32(self.episodes))
        return out
