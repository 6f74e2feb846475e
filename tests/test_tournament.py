"""bppo.tournament on the CPU: the reference's own known answers (tournament.rs tests, cited
per test), hand-worked pairings, whole Swiss tournaments with a deterministic engine, the
results file against a golden text, and a small tournament played by the CPU restatement of
run_stats_mode_env (the case tests/test_gpu_tournament.py repeats on the device)."""
import json
import math
import os

import pytest

import bppo
from bppo import Contestant

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tournament_results.json")


def _named(names, seeds=None):
    return [Contestant(n, initial_seed=0.0 if seeds is None else float(seeds[i])) for i, n in enumerate(names)]


def _once_each(pods, n):
    seen = sorted(i for pod in pods for i in pod)
    return seen == sorted(set(seen)) and all(0 <= i < n for i in seen)


# --------------------------------------------------- the reference's swiss_pods tests ---
def test_swiss_pods_2player():                                   # tournament.rs:2874-2894
    pods = bppo.swiss_pods(_named("ABCD"), 2)
    assert len(pods) == 2 and _once_each(pods, 4) and len(sum(pods, [])) == 4
    assert pods == [[0, 2], [1, 3]]          # equal seeds: the stable sort keeps the order; top half v bottom half


def test_swiss_pods_4player():                                   # tournament.rs:2897-2909
    pods = bppo.swiss_pods(_named("ABCD"), 4)
    assert len(pods) == 1 and len(pods[0]) == 4


def test_swiss_pods_with_different_seeds():                      # tournament.rs:2912-2924
    pods = bppo.swiss_pods(_named(["High", "Low", "Medium", "MidHigh"], [30.0, 15.0, 25.0, 28.0]), 2)
    assert len(pods) == 2
    assert pods == [[0, 2], [3, 1]]          # ranked High, MidHigh, Medium, Low


def test_swiss_pods_prefers_unfaced_opponents():                 # tournament.rs:2927-2947
    cs = _named("ABCD")
    cs[0].opponents_faced.append(1)
    cs[1].opponents_faced.append(0)
    pods = bppo.swiss_pods(cs, 2)
    a_pod = next(pod for pod in pods if 0 in pod)
    assert (a_pod[1] if a_pod[0] == 0 else a_pod[0]) in (2, 3)


def test_swiss_pods_odd_number():                                # tournament.rs:2950-2960
    assert len(bppo.swiss_pods(_named("ABC"), 2)) == 1


def test_swiss_pods_all_faced():                                 # tournament.rs:3716-3733
    cs = _named("ABCD")
    for i, c in enumerate(cs):
        c.opponents_faced = [j for j in range(4) if j != i]
    pods = bppo.swiss_pods(cs, 2)
    assert len(pods) == 2
    assert pods == [[0, 2], [1, 3]]          # no candidate is better: see test_all_faced_swap_rule


def test_swiss_pods_too_few():                                   # tournament.rs:772-774
    assert bppo.swiss_pods(_named("AB"), 4) == []


def test_contestant_new():                                       # tournament.rs:4095-4105
    c = Contestant("Test", initial_seed=42.5)
    assert c.swiss_points == 0.0 and not c.has_bye and abs(c.initial_seed - 42.5) < 2.0 ** -52
    assert c.opponents_faced == [] and c.placement_counts == [] and c.games_played == 0 and c.draw_count == 0


def test_swiss_pods_dutch_style_round_1_2player():               # tournament.rs:4108-4125
    pods = bppo.swiss_pods(_named(["Seed3", "Seed1", "Seed4", "Seed2"], [3.0, 1.0, 4.0, 2.0]), 2)
    assert len(pods) == 2 and all(len(p) == 2 for p in pods)
    assert pods == [[2, 3], [0, 1]]          # ranked Seed4, Seed3, Seed2, Seed1: 4 v 2, 3 v 1


def test_swiss_pods_dutch_style_round_1():                       # tournament.rs:4128-4146
    cs = [Contestant(f"Player{i}", initial_seed=float(i)) for i in range(8)]
    pods = bppo.swiss_pods(cs, 4)
    assert len(pods) == 2 and all(len(p) == 4 for p in pods)
    assert pods == [[7, 5, 3, 1], [6, 4, 2, 0]]     # ranks [0, 2, 4, 6] and [1, 3, 5, 7] by seed position


def test_swiss_pods_subsequent_rounds():                         # tournament.rs:4149-4171
    cs = _named("ABCD", [1.0, 2.0, 3.0, 4.0])
    for c, p in zip(cs, (2.0, 1.0, 0.5, 0.0)):
        c.swiss_points = p
    pods = bppo.swiss_pods(cs, 2)
    assert len(pods) == 2 and any(0 in pod for pod in pods)
    # four brackets of one: A floats to B, C floats to D
    assert pods == [[0, 1], [2, 3]]


# -------------------------------------------------------------- hand-worked pairings ---
def test_all_faced_swap_rule():
    """every pairing is a repeat: pod 0 = [0, 2] tries [0, 3], which repeats too, and stays"""
    cs = _named("ABCD")
    for i, c in enumerate(cs):
        c.opponents_faced = [j for j in range(4) if j != i]
    assert bppo.form_dutch_pods_with_floaters([0, 1, 2, 3], 2, cs) == ([[0, 2], [1, 3]], [])


def test_floater_joins_the_next_bracket_at_the_top():
    cs = _named("ABCDEF", [6, 5, 4, 3, 2, 1])
    for c, p in zip(cs, (2.0, 2.0, 2.0, 1.0, 1.0, 1.0)):
        c.swiss_points = p
    # bracket {0, 1, 2}: one pod [0, 1], 2 floats; bracket {3, 4, 5} becomes [2, 3, 4, 5]: 2 v 4, 3 v 5
    assert bppo.swiss_pods(cs, 2) == [[0, 1], [2, 4], [3, 5]]
    # scores 0.001 apart or less share a bracket, more do not
    cs[3].swiss_points = 1.0005
    assert bppo.swiss_pods(cs, 2) == [[0, 1], [2, 4], [3, 5]]
    cs[3].swiss_points = 1.002
    # brackets {0,1,2}, {3}, {4,5}: [0,1]; pool [2,3]: [2,3]; pool [4,5]: [4,5]
    assert bppo.swiss_pods(cs, 2) == [[0, 1], [2, 3], [4, 5]]


def test_leftover_floaters_of_the_last_bracket_do_not_play():
    cs = _named("ABCDE", [5, 4, 3, 2, 1])
    for c, p in zip(cs, (2.0, 2.0, 1.0, 1.0, 1.0)):
        c.swiss_points = p
    pods = bppo.swiss_pods(cs, 2)
    assert pods == [[0, 1], [2, 3]] and not any(4 in p for p in pods)
    assert bppo.form_dutch_pods_with_floaters([2, 3, 4], 2, cs) == ([[2, 3]], [4])
    assert bppo.form_dutch_pods_with_floaters([4], 2, cs) == ([], [4])


def test_swap_that_succeeds():
    cs = _named("ABCD")
    cs[0].opponents_faced.append(2)
    cs[2].opponents_faced.append(0)
    # pod 0 = [0, 2] repeats; the next of the last group, 3, does not: swapped, and pod 1 gets 2
    assert bppo.swiss_pods(cs, 2) == [[0, 3], [1, 2]]
    assert bppo.has_repeat_opponents([0, 2], cs) and not bppo.has_repeat_opponents([0, 3], cs)
    # pods of three: only the last group's player is exchanged
    cs = _named("ABCDEF")
    cs[0].opponents_faced.append(4)
    assert bppo.swiss_pods(cs, 3) == [[0, 2, 5], [1, 3, 4]]


def test_no_swap_exists_and_the_repeat_stands():
    cs = _named("ABCD")
    cs[1].opponents_faced.append(3)
    cs[3].opponents_faced.append(1)
    # the last pod has no later player of the last group to swap with
    assert bppo.swiss_pods(cs, 2) == [[0, 2], [1, 3]]
    # a repeat inside the first groups is not repaired either: 0 met 2 and 3
    cs = _named("ABCDEF")
    cs[0].opponents_faced.append(2)
    assert bppo.swiss_pods(cs, 3) == [[0, 2, 4], [1, 3, 5]]
    # only the earlier player's list is read (tournament.rs:753-762)
    cs = _named("AB")
    cs[1].opponents_faced.append(0)
    assert not bppo.has_repeat_opponents([0, 1], cs) and bppo.has_repeat_opponents([1, 0], cs)


def test_byes_are_not_repeated_while_somebody_has_none():
    cs = _named("ABC", [3, 2, 1])
    got = [bppo.assign_byes(cs, 2) for _ in range(4)]
    # lowest (points, seed) without a bye: C; then B (0 points) before A; then A; then nobody is left
    assert got == [[2], [1], [0], []]
    assert [c.swiss_points for c in cs] == [1.0, 1.0, 1.0] and all(c.has_bye for c in cs)
    # points come first: the lowest seed, ahead on points, is passed over
    cs = _named("ABC", [3, 2, 1])
    cs[2].swiss_points = 1.0
    assert bppo.assign_byes(cs, 2) == [1]
    assert bppo.assign_byes(_named("ABCD"), 2) == []


def test_three_byes_with_11_contestants_and_pods_of_four():
    cs = [Contestant(f"c{i}", initial_seed=float(i)) for i in range(11)]
    cs[0].swiss_points = 3.0                     # the lowest seed is ahead on points
    byes, pods = bppo.round_pods(cs, 4)
    assert byes == [1, 2, 3]
    assert [c.swiss_points for c in cs[:4]] == [3.0, 3.0, 3.0, 3.0] and [c.has_bye for c in cs[:5]] == [False, True, True, True, False]
    # the 8 others, ranked (points, seed) descending: 0 | 10, 9, 8, 7, 6, 5, 4.  Bracket {0} floats
    # to the top of the next: [0, 10, 9, 8, 7, 6, 5, 4] -> two pods of every second
    assert pods == [[0, 9, 7, 5], [10, 8, 6, 4]]


# ----------------------------------------- the reference's update-stats tests (2567-2697) ---
def _play(cs, pod, games):
    bppo.update_stats_from_games(cs, pod, games)
    from bppo.tournament import compute_tournament_ratings
    return compute_tournament_ratings(cs, [(pod, g) for g in games], device=None, backend="host").ratings


def test_update_ratings_win():                                   # tournament.rs:2567-2592
    cs = _named("AB")
    r = _play(cs, [0, 1], [[1, 2]])
    assert r[0].rating > r[1].rating and abs(r[1].rating - 1000.0) < 1.0     # the last contestant is the anchor
    assert (cs[0].wins(), cs[0].losses(), cs[1].wins(), cs[1].losses()) == (1, 0, 0, 1)


def test_update_ratings_loss():                                  # tournament.rs:2595-2613
    cs = _named("AB")
    _play(cs, [0, 1], [[2, 1]])
    assert cs[0].losses() == 1 and cs[1].wins() == 1


def test_update_ratings_draw():                                  # tournament.rs:2616-2636
    cs = _named("AB")
    r = _play(cs, [0, 1], [[1, 1]])
    assert abs(r[0].rating - r[1].rating) < 50.0 and cs[0].draws() == 1 and cs[1].draws() == 1
    assert [c.swiss_points for c in cs] == [0.5, 0.5]


def test_update_ratings_tracks_opponents():                      # tournament.rs:2639-2656
    cs = _named("AB")
    _play(cs, [0, 1], [[1, 2]])
    assert 1 in cs[0].opponents_faced and 0 in cs[1].opponents_faced


def test_update_ratings_multiple_games():                        # tournament.rs:2659-2697
    cs = _named("AB")
    r = _play(cs, [0, 1], [[1, 2], [1, 2], [1, 2], [2, 1], [1, 1]])
    assert r[0].rating > r[1].rating
    assert (cs[0].wins(), cs[0].losses(), cs[0].draws()) == (3, 1, 1)
    assert (cs[1].wins(), cs[1].losses(), cs[1].draws()) == (1, 3, 1)
    assert cs[0].placement_counts == [4, 1] and cs[0].games_played == 5
    assert [c.swiss_points for c in cs] == [1.0, 0.0]             # one match: 3.5 v 1.5 game points -> places 1, 2


def test_match_points_ties_and_pods_of_four():
    cs = _named("ABCD")
    # game points: A 3 + 0, B 2 + 1, C 1 + 2, D 0 + 3: all 3.0 -> every match placement 1 -> 1.5 each
    bppo.update_stats_from_games(cs, [0, 1, 2, 3], [[1, 2, 3, 4], [4, 3, 2, 1]])
    assert [c.swiss_points for c in cs] == [1.5] * 4 and [c.draw_count for c in cs] == [0] * 4
    assert cs[0].placement_counts == [1, 0, 0, 1] and cs[0].opponents_faced == [1, 2, 3] and cs[2].opponents_faced == [0, 1, 3]
    # A and B tie for first on game points: places 1, 1, 3, 4 -> 2.5, 2.5, 1, 0
    cs = _named("ABCD")
    bppo.update_stats_from_games(cs, [3, 1, 2, 0], [[1, 2, 3, 4], [2, 1, 3, 4]])
    assert [c.swiss_points for c in cs] == [0.0, 2.5, 1.0, 2.5]
    assert cs[3].opponents_faced == [1, 2, 0]                      # first-met order, the pod's order
    bppo.update_stats_from_games(cs, [3, 1, 2, 0], [])             # no games: nothing happens
    assert cs[3].games_played == 2


def test_pod_summaries():                                        # tournament.rs:54-106
    games = [[1, 2], [2, 1], [1, 1]]
    assert bppo.pod_avg_points(games, 0) == 0.5 and bppo.pod_avg_points([], 0) == 0.0
    assert bppo.pod_full_draws(games) == 1
    assert bppo.pod_summary(games, ["A", "B"]) == "A vs B: 0.50-0.50 (draw)"
    assert bppo.pod_summary([[1, 2], [1, 2], [2, 1]], ["A", "B"]) == "A vs B: 0.67-0.33 (A)"
    assert bppo.pod_summary([[2, 1]], ["A", "B"]) == "A vs B: 0.00-1.00 (B)"


# ------------------------------------------------------------------------- format ---
def test_format_selection_and_default_rounds():                  # tournament.rs:2025-2035
    assert math.comb(10, 2) == 45 and math.comb(11, 2) == 55
    assert bppo.tournament_format(10, 2) == (False, 1)
    assert bppo.tournament_format(11, 2) == (True, 5)             # ceil(log2 11) + 1
    # C(n, P) at exactly 50 and 51: C(50, 1) and C(51, 1)
    assert bppo.tournament_format(50, 1) == (False, 1)
    assert bppo.tournament_format(51, 1) == (True, 7)
    assert math.comb(8, 4) == 70 and bppo.tournament_format(8, 4) == (True, 4)
    assert bppo.tournament_format(16, 2) == (True, 5) and bppo.tournament_format(17, 2) == (True, 6)
    assert bppo.tournament_format(64, 2, rounds=3) == (True, 3)
    assert bppo.tournament_format(64, 2, "round-robin") == (False, 1)
    assert bppo.tournament_format(6, 2, "swiss") == (True, 4)
    with pytest.raises(ValueError):
        bppo.tournament_format(6, 2, "knockout")


# --------------------------------------------- whole tournaments, deterministic engine ---
def _engine(ngames=3):
    """the lower contestant index wins; game g of a pod is a full draw when (sum of the pod's
    indices + g) is a multiple of 5 (at most one game in three: the lower index wins the match)"""
    def engine(pods, seeds):
        assert len(seeds) == len(pods)
        out = []
        for pod in pods:
            order = sorted(pod)
            out.append([[1] * len(pod) if (sum(pod) + g) % 5 == 0 else [order.index(c) + 1 for c in pod]
                        for g in range(ngames)])
        return out
    return engine


def _tournament(n, cfg, rounds):
    cs = [Contestant(f"c{i}", initial_seed=float(100 - i)) for i in range(n)]
    res = bppo.run_tournament(cfg, cs, [], None, 3, 1, seed=5, rounds=rounds, format="swiss", engine=_engine(),
                              rating_backend="host", device=None)
    return cs, res, [[p for r, p, g in res.pods if r == rd] for rd in range(1, rounds + 1)]


def test_swiss_tournament_9_contestants_pods_of_2():
    """Worked by hand; c_i has seed 100 - i, so ranking by seed is ranking by index.
    Round 1: the bye goes to 8; top half v bottom half.  Round 2: bye 7 (lowest of the pointless
    without one); brackets {0,1,2,3,8} and {4,5,6}: 8 floats to the top of the second.  Round 3:
    bye 6; {0,1}, {2,3,4,5,7,8}.  The active contestants are paired by their position among the
    active ones while opponents_faced lists table indices (as the reference does), so after a
    bye the repeat check misses 3 v 7 (position 6 is contestant 7).  Round 4: bye 5; 0 floats
    into {1,2,3,4}: [0,2] is a repeat and swaps to [0,3]; in the last bracket [4,7 at position
    6] is taken for a repeat (4 met contestant 6) and swaps to 4 v 8, a real repeat."""
    cs, res, pods = _tournament(9, {"env": "connect_four"}, 4)
    assert res.use_swiss and res.num_rounds == 4
    assert res.byes == [[8], [7], [6], [5]]
    assert pods == [[[0, 4], [1, 5], [2, 6], [3, 7]],
                    [[0, 2], [1, 3], [8, 5], [4, 6]],
                    [[0, 1], [2, 5], [3, 7], [4, 8]],
                    [[0, 3], [1, 2], [4, 8], [6, 7]]]
    assert [c.swiss_points for c in cs] == [4.0, 3.0, 2.0, 2.0, 3.0, 2.0, 2.0, 1.0, 1.0]
    assert [c.opponents_faced for c in cs] == [[4, 2, 1, 3], [5, 3, 0, 2], [6, 0, 5, 1], [7, 1, 0], [0, 6, 8],
                                               [1, 8, 2], [2, 4, 7], [3, 6], [5, 4]]
    assert [c.has_bye for c in cs] == [False] * 5 + [True] * 4
    assert [c.games_played for c in cs] == [12, 12, 12, 12, 12, 9, 9, 9, 9]
    assert res.standings() == [0, 1, 4, 2, 3, 5, 6, 7, 8]
    # one seed per pod in play order from StdRng(5)
    rng = bppo.StdRng.seed_from_u64(5)
    assert res.pod_seeds == [rng.next_u64() for _ in range(16)] and len(set(res.pod_seeds)) == 16
    assert [len(g) for _, _, g in res.pods] == [3] * 16
    assert len(res.ratings.ratings) == 9 and abs(res.ratings.ratings[8].rating - 1000.0) < 1e-6     # anchor: the last


def test_swiss_tournament_7_contestants_pods_of_3():
    """Round 1: bye 6; [0,2,4], [1,3,5].  Points 2, 2, 1, 1, 0, 0, bye 2.  Round 2: bye 5; active
    0,1,2,3,4,6 ranked 0, 1, 6 | 2, 3 | 4: pod [0,1,6]; 2, 3 float to 4: [2,3,4].  Round 3: bye 4."""
    cs, res, pods = _tournament(7, {"env": "skull", "player_count": 3}, 3)
    assert res.byes == [[6], [5], [4]]
    assert pods == [[[0, 2, 4], [1, 3, 5]], [[0, 1, 6], [2, 3, 4]], [[0, 1, 2], [3, 5, 6]]]
    assert [c.swiss_points for c in cs] == [6.0, 4.0, 3.0, 4.0, 2.0, 3.0, 2.0]
    assert [c.opponents_faced for c in cs] == [[2, 4, 1, 6], [3, 5, 0, 6, 2], [0, 4, 3, 1], [1, 5, 2, 4, 6],
                                               [0, 2, 3], [1, 3, 6], [0, 1, 3, 5]]
    assert [c.placement_counts for c in cs] == [[9, 0, 0], [4, 5, 0], [4, 3, 2], [5, 4, 0], [1, 0, 5], [2, 2, 2],
                                                [1, 0, 5]]
    assert res.standings() == [0, 1, 3, 2, 5, 4, 6]


def test_round_robin_tournament():
    cs = [Contestant(f"c{i}", initial_seed=float(i)) for i in range(4)]
    res = bppo.run_tournament({"env": "connect_four"}, cs, [], None, 3, 1, seed=1, engine=_engine(),
                              rating_backend="host", device=None)
    assert not res.use_swiss and res.num_rounds == 1 and res.byes == [[]]
    assert [(r, p) for r, p, g in res.pods] == [(1, p) for p in bppo.round_robin_pods(4, 2)]
    assert [c.swiss_points for c in cs] == [3.0, 2.0, 1.0, 0.0]


def test_split_round():
    from bppo.tournament import split_round
    pods = [[0, 1], [2, 3], [0, 2], [4, None], [None, 5], [6, 7]]
    assert split_round(pods, 4) == [(0, 3), (3, 5), (5, 6)]
    assert split_round(pods, 64) == [(0, 6)]
    assert split_round(pods, 64, max_pods=4) == [(0, 4), (4, 6)]
    assert split_round([], 4) == []
    with pytest.raises(ValueError):
        split_round([[0, 1, 2]], 2)


# ------------------------------------------------------------------ the results file ---
def _fixed_result():
    """tournament.rs:2963-3043 test_build_results, grown by a third contestant"""
    from bppo.ratings import PlayerRating, RatingResult
    cs = [Contestant("Winner", initial_seed=0.0, source="runs/a/checkpoints/step_00000100"),
          Contestant("Loser", initial_seed=0.0), Contestant("Mid", initial_seed=2.0)]
    cs[0].placement_counts, cs[0].games_played, cs[0].swiss_points = [4, 1], 5, 1.5
    cs[1].placement_counts, cs[1].games_played = [0, 3], 3
    cs[2].placement_counts, cs[2].games_played, cs[2].draw_count, cs[2].swiss_points = [2, 0], 2, 1, 0.5
    ratings = RatingResult([PlayerRating(1400.0, 100.0), PlayerRating(1000.0, 100.0), PlayerRating(1234.5678, 87.25)])
    pods = [(1, [0, 1], [[1, 2], [1, 2], [1, 2]]), (2, [0, 2], [[1, 1], [2, 1]])]
    return bppo.TournamentResult(contestants=cs, pods=pods, byes=[[2], [1]], ratings=ratings, num_rounds=2,
                                 use_swiss=True, num_games=3, temp=0.4, seed=42, environment="connect_four")


def test_build_results():                                        # tournament.rs:2963-3113, 3638-3713
    res = _fixed_result()
    r = res.results("unix:1700000000")
    assert list(r) == ["rankings", "pods", "config", "environment", "timestamp"]
    assert [e["name"] for e in r["rankings"]] == ["Winner", "Mid", "Loser"]
    assert [e["rank"] for e in r["rankings"]] == [1, 2, 3]
    assert list(r["rankings"][0]) == ["rank", "name", "source", "swiss_points", "rating", "uncertainty", "rating_low",
                                      "rating_high", "placement_counts", "draw_count", "games_played"]
    assert "source" not in r["rankings"][1] and "source" not in r["rankings"][2]
    assert r["rankings"][0]["rating_low"] == 1200.0 and r["rankings"][0]["rating_high"] == 1600.0
    assert len(r["pods"]) == 2 and [p["round"] for p in r["pods"]] == [1, 2] and r["pods"][1]["draws"] == 1
    assert r["pods"][0] == {"round": 1, "contestants": ["Winner", "Loser"], "avg_points": [1.0, 0.0], "games": 3, "draws": 0}
    assert r["pods"][1]["avg_points"] == [0.25, 0.75]
    assert r["environment"] == "connect_four" and r["config"]["num_games_per_matchup"] == 3 and r["config"]["seed"] == 42
    assert list(r["config"]) == ["num_games_per_matchup", "num_rounds", "format", "temp", "seed"]
    assert r["config"]["format"] == "swiss"
    res.use_swiss, res.temp, res.seed = False, None, None
    r = res.results()
    assert r["config"] == {"num_games_per_matchup": 3, "num_rounds": 2, "format": "round-robin"}
    assert r["timestamp"].startswith("unix:") and int(r["timestamp"][5:]) > 0       # tournament.rs:2556-2563


def test_results_json_golden():
    text = _fixed_result().results_json("unix:1700000000")
    with open(GOLDEN) as f:
        want = f.read()
    assert text == want.rstrip("\n")
    back = json.loads(text)
    assert back == json.loads(json.dumps(_fixed_result().results("unix:1700000000")))
    assert '"temp": 0.4,' in text and '"swiss_points": 1.5,' in text and '"rating": 1400.0,' in text


# ----------------------------------------------- a small tournament on the restatement ---
def test_small_tournament_on_the_cpu_restatement():
    from test_gpu_eval import MAX_STEPS
    from tournament_cases import SMALL, small_cpu
    res, cpu = small_cpu()
    assert res.use_swiss and res.num_rounds == 3
    assert [len(b) for b in res.byes] == [1, 1, 1] and len({b[0] for b in res.byes}) == 3
    assert len(res.pods) == 9 == len(cpu.runs)
    # every pod ends by num_games, well inside max_steps: the device comparison cannot pass on truncated runs
    for run, (rnd, pod, games) in zip(cpu.runs, res.pods):
        assert run["ended_by"] == "num_games" and len(run["games"]) == SMALL["games"] == len(games)
        assert run["steps"] * 4 < MAX_STEPS and run["max_len"] * 4 < MAX_STEPS
    for rd in (1, 2, 3):
        played = sorted(i for r, pod, _ in res.pods if r == rd for i in pod) + res.byes[rd - 1]
        assert sorted(played) == list(range(7))
    cs = res.contestants
    assert [c.games_played for c in cs] == [SMALL["games"] * (3 - c.has_bye) for c in cs]
    assert sum(c.swiss_points for c in cs) == 3 * 3 * 1.0 + 3 * 1.0          # a point per match, one per bye
    assert all(sum(c.placement_counts) == c.games_played for c in cs)
    assert not all(g == games[0] for _, _, games in res.pods for g in games)  # not every game went one way
    rt = res.ratings
    assert abs(rt.ratings[6].rating - 1000.0) < 1e-9 and rt.stats.n_games == 9 * SMALL["games"]     # the anchor is Random
    assert len(json.loads(res.results_json())["rankings"]) == 7
