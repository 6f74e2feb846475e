"""The restatement tests/pl_ref.py reproduces plackett_luce.rs's own unit-test facts, the rating
fixtures keep clear of the convergence threshold, and tests/golden/ratings_ref.json (what the GPU
tests compare with) is what the restatement computes."""
import json
import math
import os

import pytest

import pl_ref

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ratings_ref.json")))


def test_two_to_one_wins_is_400_log10_2():
    games = [([0, 1], [1, 2])] * 20 + [([0, 1], [2, 1])] * 10
    r = pl_ref.compute_ratings(2, games, 1)
    assert abs((r.ratings[0][0] - r.ratings[1][0]) - 400.0 * math.log10(2.0)) < 1e-3
    assert r.ratings[1] == (1000.0, 0.0)                 # the anchor: exactly anchor_elo, uncertainty 0
    assert r.converged


def test_expand_with_ties():
    c = pl_ref.expand_games_to_comparisons([([0, 1, 2], [1, 1, 3])])
    assert c == [(0, [2], 0.5), (1, [2], 0.5)]


def test_expansion_complex_tie_scenario():
    c = pl_ref.expand_games_to_comparisons([([0, 1, 2, 3], [1, 2, 2, 4])])
    assert c == [(0, [1, 2, 3], 1.0), (1, [3], 0.5), (2, [3], 0.5)]


def test_player_without_games_gets_the_default():
    r = pl_ref.compute_ratings(3, [([0, 1], [1, 2]), ([0, 1], [2, 1])], 1)
    assert r.ratings[2] == (1000.0, 350.0)


def test_never_winning_player_falls_by_one_per_iteration():
    """the `gamma - 1` branch (:306-308): with 9 players the centring gives 1/9 of the step back, so
    max_change settles at 8/9 and the loop runs out of iterations.  (With few players the others'
    exp(gamma) outgrow 1 / epsilon before that, the never-winner's denominator falls under
    epsilon, the third branch holds it still and the fit converges: 73 iterations for 3 players.)"""
    r = pl_ref.reference("edge")
    assert (r.converged, r.iterations_used) == (False, 100)
    assert r.gammas[8] < -80.0 and all(abs(d - 8.0 / 9.0) < 1e-9 for d in r.deltas[50:])
    r3 = pl_ref.compute_ratings(3, [([0, 1, 2], [1, 2, 3]), ([1, 0, 2], [1, 2, 3])], 0)
    assert (r3.converged, r3.iterations_used) == (True, 73)


def test_early_returns():
    assert pl_ref.compute_ratings(0, [], 0).ratings == []
    r = pl_ref.compute_ratings(3, [], 0)
    assert r.ratings == [(1000.0, 350.0)] * 3 and (r.converged, r.iterations_used, r.final_delta) == (True, 0, 0.0)
    r = pl_ref.compute_ratings(2, [([0], [1]), ([1], [1])], 0)        # games, but no comparison
    assert r.ratings == [(1000.0, 350.0)] * 2 and r.iterations_used == 0


@pytest.mark.parametrize("name", pl_ref.FIXTURES)
def test_fixture_stays_clear_of_the_threshold(name):
    """neither backend's rounding can move the stopping iteration: the last max_change and the
    one before differ from convergence_threshold by more than 1e-9"""
    r = pl_ref.reference(name)
    for d in r.deltas[-2:]:
        assert abs(d - 1e-6) > 1e-9, (name, d)
    assert r.converged == (name != "edge")


def test_edge_fixture_is_what_it_says():
    n, games, anchor = pl_ref.fixture("edge")
    assert sorted(set(len(g[0]) for g in games)) == [1, 2, 3, 6]
    assert any(sorted(g[1])[:3] == [1, 1, 1] for g in games)                       # a three-way tie for first
    assert any(len(g[1]) > 2 and sorted(g[1])[-2] == sorted(g[1])[-1] > 1 for g in games)   # a tie for last
    played = pl_ref.count_games_per_player(games, n)
    assert played[7] == 0 and all(played[i] > 0 for i in range(n) if i != 7)
    assert not any(w == 8 for w, _, _ in pl_ref.expand_games_to_comparisons(games)) and played[8] > 0
    assert 0 < anchor < n - 1


@pytest.mark.parametrize("name", pl_ref.FIXTURES)
def test_golden_file_is_the_restatement(name):
    r, g = pl_ref.reference(name), GOLDEN[name]
    assert [x[0] for x in r.ratings] == g["rating"] and [x[1] for x in r.ratings] == g["uncertainty"]
    assert r.gammas == g["gamma"] and r.final_delta == g["final_delta"]
    assert (r.converged, r.iterations_used, r.n_comparisons) == (g["converged"], g["iterations_used"], g["n_comparisons"])
    if name in ("A", "M", "six", "long", "edge"):            # the cheap ones; D and N130 take 20 s of pure Python
        assert pl_ref.order_spread(name) == g["spread"]
    assert g["spread"]["iterations"] == [g["iterations_used"]]     # no ordering moved the stopping iteration
