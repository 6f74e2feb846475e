"""The rating table's host backend (bppo_ratings_fit backend 1; no GPU) equals the restatement
tests/pl_ref.py bit for bit; weight / split invariants; RatingHistory, find_anchor_index and the
struct sizes."""
import ctypes as C

import numpy as np
import pytest

import bppo
import bppo._lib as L
import pl_ref
from bppo.ratings import PlackettLuceConfig, RatingTable, compute_ratings


def _split(games):
    return [g[0] for g in games], [g[1] for g in games]


def _bits(res):
    return ([r.rating for r in res.ratings], [r.uncertainty for r in res.ratings], list(res.gammas),
            res.stats.converged, res.stats.iterations_used, res.stats.final_delta)


def _host_fit(n, games, anchor, weight=None, pieces=1):
    pl, pc = _split(games)
    with RatingTable(device=None) as t:
        cuts = [len(games) * k // pieces for k in range(pieces + 1)]
        for lo, hi in zip(cuts, cuts[1:]):
            t.add_games(pl[lo:hi], pc[lo:hi], None if weight is None else weight[lo:hi])
        assert t.num_games == len(games)
        return t.fit(n, anchor, backend="host")


def test_struct_sizes():
    assert L.lib().bppo_pl_config_size() == C.sizeof(L.PlConfig) == 40
    assert L.lib().bppo_pl_stats_size() == C.sizeof(L.PlStats) == 40


@pytest.mark.parametrize("name", pl_ref.FIXTURES)
def test_host_backend_is_the_restatement(name):
    n, games, anchor = pl_ref.fixture(name)
    ref = pl_ref.reference(name)
    res = _host_fit(n, games, anchor)
    assert _bits(res) == ([r[0] for r in ref.ratings], [r[1] for r in ref.ratings], ref.gammas, ref.converged,
                          ref.iterations_used, ref.final_delta)
    assert (res.stats.n_games, res.stats.n_comparisons) == (len(games), ref.n_comparisons)


def test_padded_arrays_equal_ragged_lists():
    n, games, anchor = pl_ref.fixture("M")
    pl = np.full((len(games), 6), -1, np.int32)
    pc = np.zeros((len(games), 6), np.int32)
    for g, (a, b) in enumerate(games):
        pl[g, :len(a)], pc[g, :len(b)] = a, b
    with RatingTable(device=None) as t:
        t.add_games(pl, pc)
        assert _bits(t.fit(n, anchor, backend="host")) == _bits(_host_fit(n, games, anchor))


def test_split_add_calls_give_identical_bits():
    n, games, anchor = pl_ref.fixture("D")
    assert _bits(_host_fit(n, games, anchor, pieces=4)) == _bits(_host_fit(n, games, anchor))


def test_weight_three_equals_three_copies():
    """within 16 x the restatement's own order spread on this fixture (weighting a comparison by 3
    and listing it three times differ in the sums' rounding only)"""
    n, games, anchor = pl_ref.fixture("M")
    w = [1.0] * len(games)
    w[5] = 3.0
    a = _host_fit(n, games, anchor, weight=w)
    b = _host_fit(n, games[:6] + [games[5], games[5]] + games[6:], anchor)
    ref = pl_ref.compute_ratings(n, games, anchor, weights=w)
    assert _bits(a)[:2] == ([r[0] for r in ref.ratings], [r[1] for r in ref.ratings])
    sp = pl_ref.order_spread("M")
    assert a.stats.iterations_used == b.stats.iterations_used
    assert max(abs(x.rating - y.rating) for x, y in zip(a.ratings, b.ratings)) <= 16 * sp["rating"]
    assert max(abs(x.uncertainty - y.uncertainty) for x, y in zip(a.ratings, b.ratings)) <= 16 * sp["uncertainty"]


def test_early_returns_and_config():
    with RatingTable(device=None) as t:
        r = t.fit(0, 0, backend="host")
        assert r.ratings == [] and (r.stats.converged, r.stats.iterations_used) == (True, 0)
        r = t.fit(3, 0, backend="host")
        assert [(x.rating, x.uncertainty) for x in r.ratings] == [(1000.0, 350.0)] * 3
        t.add_games([[0], [1]], [[1], [1]])                   # games without a comparison
        r = t.fit(2, 0, PlackettLuceConfig(anchor_elo=1200.0), backend="host")
        assert [(x.rating, x.uncertainty) for x in r.ratings] == [(1200.0, 350.0)] * 2
        assert (r.stats.n_games, r.stats.n_comparisons, r.stats.iterations_used) == (2, 0, 0)
    n, games, anchor = pl_ref.fixture("six")
    cfg = PlackettLuceConfig(max_iterations=7, anchor_elo=1500.0, ci_inflation_factor=1.0)
    ref = pl_ref.compute_ratings(n, games, 3, pl_ref.Config(max_iterations=7, anchor_elo=1500.0, ci_inflation_factor=1.0))
    res = compute_ratings(n, games, 3, cfg, device=None)
    assert _bits(res)[:2] == ([r[0] for r in ref.ratings], [r[1] for r in ref.ratings])
    assert (res.stats.converged, res.stats.iterations_used) == (False, 7)
    assert res.ratings[3].confidence_interval() == (1500.0, 1500.0)


def test_argument_errors_on_the_host():
    with RatingTable(device=None) as t:
        def bad(msg, fn):
            with pytest.raises(bppo.BppoError) as e:
                fn()
            assert e.value.status == L.ERR_ARG and msg in str(e.value), str(e.value)
        bad("P outside 1..6", lambda: t.add_games(np.zeros((1, 7), np.int32), np.ones((1, 7), np.int32)))
        bad("placement < 1", lambda: t.add_games([[0, 1]], [[1, 0]]))
        bad("weight", lambda: t.add_games([[0, 1]], [[1, 2]], [-1.0]))
        bad("weight", lambda: t.add_games([[0, 1]], [[1, 2]], [float("inf")]))
        bad("after a -1", lambda: t.add_games(np.array([[0, -1, 2]], np.int32), np.ones((1, 3), np.int32)))
        assert t.num_games == 0
        t.add_games([[0, 5]], [[1, 2]])
        bad("anchor outside", lambda: t.fit(6, 6, backend="host"))
        bad(">= num_players", lambda: t.fit(5, 0, backend="host"))
        bad("num_players > 1024", lambda: t.fit(1025, 0, backend="host"))
        bad("host-only", lambda: t.fit(6, 0, backend="device"))
        bad("host-only", lambda: t.add_completions(type("Ctx", (), {"h": None})(), 0, [0]))


def test_find_anchor_index():
    f = bppo.find_anchor_index
    assert f(["step_00000200", "Random", "step_00000100"]) == 1
    assert f(["step_00000200", "best", "step_00000100", "step_00000100"]) == 2
    assert f(["best", "latest"]) is None and f([]) is None


def _history_restatement(games, idx_of, steps, first_idx):
    """rating_history.rs:270-341 on the restatement"""
    n = len(idx_of)
    pl_games = [([idx_of[cur]] + [idx_of[o] for o in opps], list(places)) for cur, opps, places in games]
    raw = [r[0] for r in pl_ref.compute_ratings(n, pl_games, 0).ratings]
    adjusted = [r + (1000.0 - raw[first_idx]) for r in raw]
    best_idx = max(range(n), key=lambda i: (adjusted[i], -i))
    return dict(current_elo=adjusted[max(n - 2, 0)], best_elo=adjusted[best_idx], best_step=steps[best_idx],
                total_games=len(games))


def test_rating_history_matches_the_reference_rules():
    """4 checkpoints, 40 hand-made games; the learner plays as "step_00000000" before the first
    save and is registered first, so the first saved checkpoint (the 1000 anchor) is player 1"""
    import random
    rng = random.Random(5)
    h = bppo.RatingHistory(device=None)
    assert h.compute_ratings() == dict(current_elo=1000.0, best_elo=1000.0, best_step=0, total_games=0)
    names = ["step_00001000", "step_00002000", "step_00003000", "step_00004000"]
    games, cur = [], "step_00000000"
    for k, name in enumerate(names):
        for _ in range(10):
            opps = [rng.choice(names[:k] or ["step_00000000"]) for _ in range(rng.choice((1, 2, 3)))]
            places = [rng.randint(1, len(opps) + 1) for _ in range(len(opps) + 1)]
            places[rng.randrange(len(places))] = 1
            if k == 0:
                opps = ["step_00001000"]          # before the first save: the pool's only member
            games.append((h.current_checkpoint or "step_00000000", opps, places[:len(opps) + 1]))
            h.record_game(*games[-1])
        h.on_checkpoint_saved(name, (k + 1) * 1000)
    assert h.idx_to_checkpoint == ["step_00000000"] + names and h.first_checkpoint_idx == 1
    assert h.total_games == 40
    want = _history_restatement(games, h.checkpoint_to_idx, h.idx_to_step, 1)
    assert h.compute_ratings() == want
    assert h.cached_ratings[1] == 1000.0 and want["best_step"] in (0, 1000, 2000, 3000, 4000)
    h.close()
