"""The reference's episode logging restated line by line (burn-ppo main.rs:842-875,
main.rs:1134-1217, env.rs:208-261), f32 where the reference is f32, and the synthetic
episode sets the episode-statistics tests share.

An episode here is a dict: total_rewards (list of f32, one per player), length, env_index,
step, outcome (GameOutcome's placements, one per seat of the game, or None)."""
import math
from collections import deque

import numpy as np

f32 = np.float32


# ------------------------------------------------------------- env.rs:208-261 ---
def compute_avg_points(outcomes, max_players):
    if len(outcomes) == 0:
        return [f32(0.0)] * max_players, [0] * max_players, f32(0.0)
    total_points = [0.0] * max_players                       # f64
    game_counts = [0] * max_players
    draws = 0
    for placements in outcomes:
        if all(p == 1 for p in placements):
            draws += 1
        n = len(placements)
        for player, place in enumerate(placements):
            if player >= max_players:
                break
            tied_count = sum(1 for p in placements if p == place)
            avg_position = float(place) + (float(tied_count) - 1.0) / 2.0
            points = float(n) - avg_position
            total_points[player] += points
            game_counts[player] += 1
    avg_points = [f32(pts / float(c)) if c > 0 else f32(0.0) for pts, c in zip(total_points, game_counts)]
    draw_rate = f32(draws) / f32(len(outcomes))
    return avg_points, game_counts, draw_rate


# ---------------------------------------------------------- main.rs:1134-1217 ---
def episode_scalars(episodes, num_players):
    """the scalars one log writes for the episodes since the last one, in the order the
    rollouts returned them -> {name: python float of the f32 logged}"""
    out = {}
    episodes_since_log = [(e["total_rewards"][0], e["length"]) for e in episodes]
    episodes_since_log_mp = [(e["total_rewards"], e["outcome"]) for e in episodes]
    if episodes_since_log:
        lengths = [l for _, l in episodes_since_log]
        out["episode/length_mean"] = f32(sum(lengths)) / f32(len(lengths))
        out["episode/length_max"] = f32(max(lengths))
        out["episode/length_min"] = f32(min(lengths))
        out["episode/count"] = f32(len(episodes_since_log))
    if episodes_since_log_mp:
        for player in range(num_players):
            player_returns = [f32(r[player]) if player < len(r) else f32(0.0) for r, _ in episodes_since_log_mp]
            s = f32(0.0)
            for x in player_returns:                         # iter().sum::<f32>(): sequential
                s = f32(s + x)
            mx, mn = f32(-np.inf), f32(np.inf)
            for x in player_returns:                         # fold(NEG_INFINITY, f32::max)
                mx = x if x > mx else mx
                mn = x if x < mn else mn
            out[f"episode/return_mean_p{player}"] = f32(s / f32(len(player_returns)))
            out[f"episode/return_max_p{player}"] = mx
            out[f"episode/return_min_p{player}"] = mn
        if num_players > 1:
            total_games = len(episodes_since_log_mp)
            outcomes = [o for _, o in episodes_since_log_mp if o is not None]
            avg_points, game_counts, draw_rate = compute_avg_points(outcomes, num_players)
            for player, (pts, count) in enumerate(zip(avg_points, game_counts)):
                if count > 0:
                    out[f"episode/avg_points_p{player}"] = pts
            out["episode/draw_rate"] = draw_rate
            out["episode/games_completed"] = f32(total_games)
    return {k: float(v) for k, v in out.items()}


# ------------------------------------------------------------ main.rs:842-875 ---
class Windows:
    """recent_returns, recent_returns_per_player, recent_outcomes: 100 deep"""

    def __init__(self, num_players):
        self.recent_returns = deque()
        self.recent_returns_per_player = [deque() for _ in range(num_players)]
        self.recent_outcomes = deque()

    def push(self, completed_episodes):
        """one rollout's completed episodes, in the order collect_rollouts returned them"""
        for ep in completed_episodes:
            self.recent_returns.append(ep["total_rewards"][0])
            if len(self.recent_returns) > 100:
                self.recent_returns.popleft()
            for p, reward in enumerate(ep["total_rewards"]):
                if p < len(self.recent_returns_per_player):
                    self.recent_returns_per_player[p].append(reward)
                    if len(self.recent_returns_per_player[p]) > 100:
                        self.recent_returns_per_player[p].popleft()
            if ep["outcome"] is not None:
                self.recent_outcomes.append(list(ep["outcome"]))
                if len(self.recent_outcomes) > 100:
                    self.recent_outcomes.popleft()


def rollout_order(episodes):
    """the order a rollout returns its episodes in: step by step, env order within a step
    (env.rs:470-483)"""
    return sorted(episodes, key=lambda e: (e["step"], e["env_index"]))


# --------------------------------- what the device's per-rollout block must hold ---
def stats_ref(episodes, P):
    """bppo_episode_stats of one rollout's episodes from the restatement above: the sums and
    extremes main.rs:1134-1217 reduces, the Swiss points doubled (env.rs:236-242 gives
    halves); return_sum by math.fsum (the exact sum, rounded once)"""
    n = len(episodes)
    lengths = [e["length"] for e in episodes]
    outcomes = [e["outcome"] for e in episodes if e["outcome"] is not None]
    pts2, games, draws = [0] * 6, [0] * 6, 0
    for o in outcomes:
        draws += all(p == 1 for p in o)
        for player, place in enumerate(o):
            if player >= P:
                break
            tied = sum(1 for p in o if p == place)
            points = float(len(o)) - (float(place) + (float(tied) - 1.0) / 2.0)
            assert (2.0 * points).is_integer()
            pts2[player] += int(2.0 * points)
            games[player] += 1
    rs, rmin, rmax = [0.0] * 6, [f32(np.inf)] * 6, [f32(-np.inf)] * 6
    for p in range(P):
        xs = [f32(e["total_rewards"][p]) for e in episodes]
        rs[p] = math.fsum(float(x) for x in xs)
        for x in xs:
            rmax[p] = x if x > rmax[p] else rmax[p]
            rmin[p] = x if x < rmin[p] else rmin[p]
    return dict(episodes=n, kept=n, length_sum=sum(lengths), length_min=min(lengths) if n else 2**31 - 1,
                length_max=max(lengths) if n else 0, with_outcome=len(outcomes), draws=draws, return_sum=rs,
                return_min=rmin, return_max=rmax, outcome_games=games, points2_sum=pts2)


def return_sum_bound(episodes, p):
    """|f64 sum in any order - exact sum| <= n 2^-52 sum |x|: twice the first-order bound
    (n - 1) 2^-53 sum |x| of a recursive f64 sum; 0 when the returns are integers"""
    xs = [float(f32(e["total_rewards"][p])) for e in episodes]
    if all(x.is_integer() for x in xs) and sum(abs(x) for x in xs) < 2.0**53:
        return 0.0
    return len(xs) * 2.0**-52 * math.fsum(abs(x) for x in xs)


def tail_ref(episodes, P):
    """the rollout's last 100 episodes as bppo_episode_tail dicts (bppo.episodes.tail_list)"""
    out = []
    for e in rollout_order(episodes)[-100:]:
        tr = [f32(x) for x in e["total_rewards"]] + [f32(0.0)] * (6 - len(e["total_rewards"]))
        pl = None if e["outcome"] is None else list(e["outcome"]) + [0] * (6 - len(e["outcome"]))
        out.append(dict(total_rewards=tr, length=e["length"], env_index=e["env_index"], step=e["step"], placements=pl))
    return out


def check_block(got_stats, got_tail, episodes, P, tag=""):
    """a device (or host-build) block against the restatement: integers, extremes and the
    tail exactly, return_sum within return_sum_bound"""
    want = stats_ref(episodes, P)
    for k in ("episodes", "kept", "length_sum", "length_min", "length_max", "with_outcome", "draws",
              "outcome_games", "points2_sum"):
        assert got_stats[k] == want[k], (tag, k, got_stats[k], want[k])
    for k in ("return_min", "return_max"):
        a, b = np.array(got_stats[k], f32), np.array(want[k], f32)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (tag, k, a, b)
    for p in range(6):
        err = abs(got_stats["return_sum"][p] - want["return_sum"][p])
        assert err <= return_sum_bound(episodes, p) if p < P else got_stats["return_sum"][p] == 0.0, \
            (tag, p, got_stats["return_sum"][p], want["return_sum"][p])
    tails_equal(got_tail, tail_ref(episodes, P), tag)


def tails_equal(got, want, tag=""):
    assert len(got) == len(want), (tag, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g["step"], g["env_index"], g["length"], g["placements"]) == \
               (w["step"], w["env_index"], w["length"], w["placements"]), (tag, i, g, w)
        a, b = np.array(g["total_rewards"], f32), np.array(w["total_rewards"], f32)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (tag, i, a, b)


def blocks_equal(a, b, episodes, P, tag=""):
    """two blocks of the same episodes (device against host build; pipelined against
    sequential): exact fields bit for bit, return_sum within return_sum_bound"""
    sa, ta = a
    sb, tb = b
    for k in ("episodes", "kept", "length_sum", "length_min", "length_max", "with_outcome", "draws",
              "outcome_games", "points2_sum"):
        assert sa[k] == sb[k], (tag, k, sa[k], sb[k])
    for k in ("return_min", "return_max"):
        assert np.array_equal(np.array(sa[k], f32).view(np.uint32), np.array(sb[k], f32).view(np.uint32)), (tag, k)
    for p in range(6):
        # each is an f64 sum in some order, (n - 1) 2^-53 sum |x| from the exact sum at first order
        bound = return_sum_bound(episodes, p) if p < P else 0.0
        assert abs(sa["return_sum"][p] - sb["return_sum"][p]) <= bound, (tag, p, sa["return_sum"], sb["return_sum"])
    tails_equal(ta, tb, tag)


# ------------------------------------------------------------ synthetic sets ---
def placements_from_scores(scores):
    """1 + the seats that did strictly better: ties share a placement"""
    return [1 + sum(1 for y in scores if y > x) for x in scores]


def synthetic(n, P, N, T, seed, one_step=None, integer=True, outcome="mixed", seated=None):
    """n episodes with distinct (step, env_index) keys spread over [0, T N).  one_step: all at
    that step.  integer: whole-number returns (the sums are then exact in any order), else
    arbitrary f32.  outcome: "none", "all" (random placements with ties), "mixed" (the same, a
    fifth without an outcome), "draw" (all seats first), "tie1133" (P = 4).  seated: seats of the game when
    fewer than P are dealt in (then the outcome has that many placements)."""
    rng = np.random.default_rng(seed)
    if one_step is None:
        keys = rng.choice(T * N, size=n, replace=False) if n else np.zeros(0, np.int64)
    else:
        keys = one_step * N + rng.choice(N, size=n, replace=False)
    S = seated or P
    eps = []
    for k in keys:
        if integer:
            tr = [f32(rng.integers(-3, 4)) for _ in range(P)]
        else:
            tr = [f32(rng.normal() * 10.0 ** rng.integers(-3, 3)) for _ in range(P)]
        if outcome == "none" or P == 1:
            oc = None
        elif outcome == "draw":
            oc = [1] * S
        elif outcome == "tie1133":
            oc = [1, 1, 3, 3]
        else:
            oc = None if outcome == "mixed" and rng.random() < 0.2 else \
                placements_from_scores(list(rng.integers(0, 3, S)))
        eps.append(dict(total_rewards=tr, length=int(rng.integers(1, 500)), env_index=int(k % N), step=int(k // N),
                        outcome=oc))
    return eps


# T N = 2^23: all three 11-bit digits of the tail's select are live
SYN_N, SYN_T = 4096, 2048
COUNTS = (0, 1, 99, 100, 101)


def synthetic_sets():
    """(tag, episodes, P) for every set the host-build and the device tests run"""
    sets = []
    for P in range(1, 7):
        for n in COUNTS:
            sets.append((f"P{P}-n{n}", synthetic(n, P, SYN_N, SYN_T, 100 * P + n, integer=(P + n) % 2 == 0), P))
    # the selection's worst case: every record at one step (a batch of truncations)
    sets.append(("one-step-3000", synthetic(3000, 2, SYN_N, SYN_T, 7, one_step=1234), 2))
    sets.append(("spread-3000-frac", synthetic(3000, 4, SYN_N, SYN_T, 8, integer=False), 4))
    sets.append(("all-draw", synthetic(150, 4, SYN_N, SYN_T, 9, outcome="draw"), 4))
    sets.append(("tie-1133", synthetic(150, 4, SYN_N, SYN_T, 10, outcome="tie1133"), 4))
    # Skull with 3 of its 6 seats dealt in: outcomes of 3 placements on a 6-player axis
    sets.append(("skull-3-of-6", synthetic(150, 6, SYN_N, SYN_T, 11, seated=3), 6))
    sets.append(("skull-3-seated", synthetic(150, 3, SYN_N, SYN_T, 13), 3))
    sets.append(("no-outcomes", synthetic(150, 2, SYN_N, SYN_T, 12, outcome="none"), 2))
    return sets


def scalars_equal(got, episodes, P, tag=""):
    """EpisodeWindow.scalars() against episode_scalars over the same episodes: the same keys in
    the same order; every value identical, except return_mean_p{p} where the reference's
    sequential f32 sum rounds (returns that are not whole numbers): there the window must hold
    f32(exact sum / n), and the reference lies within its own sum's first-order error
    n 2^-24 sum |x| / n of the exact mean (plus the two f32 roundings of the quotient)"""
    want = episode_scalars(episodes, P)
    assert list(got) == list(want), (tag, list(got), list(want))
    n = len(episodes)
    for k in got:
        if "return_mean_p" not in k:
            assert got[k] == want[k], (tag, k, got[k], want[k])
            continue
        p = int(k.rsplit("p", 1)[1])
        xs = [float(f32(e["total_rewards"][p])) for e in episodes]
        exact = math.fsum(xs) / n
        assert got[k] == float(f32(exact)), (tag, k, got[k], exact)
        if all(x.is_integer() for x in xs) and math.fsum(abs(x) for x in xs) < 2.0**24:
            assert got[k] == want[k], (tag, k, got[k], want[k])
        else:
            assert abs(want[k] - exact) <= 2.0**-24 * math.fsum(abs(x) for x in xs) + 2.0**-23 * abs(exact), (tag, k)
