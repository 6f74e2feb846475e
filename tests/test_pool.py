"""bppo.pool.OpponentPool: the reference's own unit tests (opponent_pool.rs:1089-1605)
restated on the Python pool, the opponent_stats.json round trip, the device-sum path
against game-by-game queue_game_result, and the sampler's determinism and distribution."""
import json
import math

import numpy as np
import pytest

from bppo.pool import OpponentPool, OpponentStats

EPS = 2.220446049250313e-16      # f64::EPSILON


def _pool(win_rates=(), alpha=0.1, exponent=1.0, seed=42, num_players=2, swiss=None, games=None):
    p = OpponentPool(num_players, alpha, exponent, seed)
    for i, w in enumerate(win_rates):
        p.add_checkpoint(f"step_{(i + 1) * 1000:08d}", (i + 1) * 1000, np.zeros(3, np.float32))
        p.available[i].win_rate = w
        if swiss is not None:
            p.available[i].avg_swiss_points = swiss[i]
        if games is not None:
            p.available[i].games_played = games[i]
    return p


def _rotation(pool, idx, wins, games, swiss_total=0.0):
    pool.pending_rotation_stats[idx] = [wins, games, swiss_total]
    pool.apply_pending_win_rate_updates()


# ---------------------------------------------------------------- stats ------
def test_opponent_stats_new():
    s = OpponentStats("step_00010000", 10000)
    assert (s.checkpoint_name, s.checkpoint_step, s.games_played) == ("step_00010000", 10000, 0)
    assert abs(s.win_rate - 0.5) < EPS and s.avg_swiss_points == 0.0


# ------------------------------------------------------------------ EMA ------
@pytest.mark.parametrize("initial,wins,games,alpha,expected", [
    (0.5, 10, 10, 0.1, 0.55),      # test_win_rate_ema_basic
    (0.5, 0, 10, 0.1, 0.45),       # test_win_rate_ema_zero_rotation
    (0.3, 8, 10, 1.0, 0.8),        # test_win_rate_ema_one_alpha
])
def test_win_rate_ema(initial, wins, games, alpha, expected):
    p = _pool([initial], alpha=alpha)
    _rotation(p, 0, wins, games)
    assert abs(p.available[0].win_rate - expected) < EPS
    assert p.available[0].games_played == games
    assert p.pending_rotation_stats == {}


def test_swiss_ema_and_games_played():
    p = _pool([0.5], alpha=0.1, num_players=4)
    _rotation(p, 0, 3, 6, 12.0)                 # rotation average 2.0 Swiss points
    assert abs(p.available[0].avg_swiss_points - 0.2) < EPS
    _rotation(p, 0, 0, 4, 0.0)
    assert abs(p.available[0].avg_swiss_points - 0.18) < 4 * EPS
    assert p.available[0].games_played == 10
    _rotation(p, 0, 0, 0, 0.0)                  # no games: untouched
    _rotation(p, 7, 1, 1, 1.0)                  # unknown pool index: ignored
    assert p.available[0].games_played == 10


def test_win_rate_convergence():
    p = _pool([0.5], alpha=0.1)
    for _ in range(100):
        _rotation(p, 0, 9, 10)
    assert abs(p.available[0].win_rate - 0.9) < 0.001


def test_win_rate_bounds():
    p = _pool([0.5], alpha=0.1)
    for _ in range(1000):
        _rotation(p, 0, 5, 5)
    assert 0.999 <= p.available[0].win_rate <= 1.0
    p = _pool([0.5], alpha=0.1)
    for _ in range(1000):
        _rotation(p, 0, 0, 5)
    assert 0.0 <= p.available[0].win_rate < 0.001


# ------------------------------------------------- selection probabilities ---
def test_selection_probability_basic():
    probs = _pool([0.2, 0.5, 0.8]).compute_all_selection_probabilities()
    for got, w in zip(probs, (0.8, 0.5, 0.2)):
        assert abs(got - w / 1.5) < 1e-10


def test_selection_probability_exponent_2():
    probs = _pool([0.2, 0.5, 0.8], exponent=2.0).compute_all_selection_probabilities()
    assert probs[0] > 0.6 and probs[2] < 0.1
    assert probs[0] > probs[1] > probs[2]
    for got, w in zip(probs, (0.64, 0.25, 0.04)):
        assert abs(got - w / 0.93) < 1e-10


def test_selection_probability_uniform_win_rates():
    for p in _pool([0.5, 0.5, 0.5]).compute_all_selection_probabilities():
        assert abs(p - 1.0 / 3.0) < EPS


def test_selection_probability_edge_win_rate_1():
    probs = _pool([0.5, 1.0, 0.3]).compute_all_selection_probabilities()
    assert abs(probs[1]) < EPS
    assert abs(probs[0] + probs[2] - 1.0) < 1e-10


def test_selection_probability_sums_to_one():
    for wr in ([0.1, 0.2, 0.3, 0.4], [0.9, 0.8, 0.7], [0.5], [0.0, 1.0], [0.33, 0.33, 0.34]):
        assert abs(sum(_pool(wr).compute_all_selection_probabilities()) - 1.0) < 1e-10, wr


def test_selection_probability_ordering():
    probs = _pool([0.1, 0.3, 0.5, 0.7, 0.9]).compute_all_selection_probabilities()
    assert all(probs[i] > probs[i + 1] for i in range(len(probs) - 1))


def test_no_nan_in_probabilities():
    for wr, exponent in (([0.0, 0.0, 0.0], 1.0), ([1.0, 1.0, 1.0], 1.0), ([0.5], 1.0), ([0.999_999, 0.000_001], 2.0)):
        probs = _pool(wr, exponent=exponent).compute_all_selection_probabilities()
        assert len(probs) == len(wr) and all(math.isfinite(p) for p in probs), (wr, exponent)
    assert _pool([1.0, 1.0, 1.0]).compute_all_selection_probabilities() == [1.0 / 3.0] * 3   # uniform fallback
    assert _pool([]).compute_all_selection_probabilities() == []


def test_weight_edges():
    p = _pool([0.0, 1.0])
    assert abs(p._weight(0.0) - 1.0) < EPS and abs(p._weight(1.0)) < EPS
    w = _pool([0.1], exponent=100.0)._weight(0.1)          # 0.9^100 ~ 2.66e-5
    assert math.isfinite(w) and 0.0 <= w < 0.001


# ----------------------------------------------------------- persistence -----
def test_opponent_stats_file_round_trip(tmp_path):
    p = _pool([0.3, 0.7], alpha=0.15, exponent=2.0, swiss=[2.5, 0.8], games=[100, 50])
    path = tmp_path / "opponent_stats.json"
    p.save_opponent_stats(path)
    doc = json.loads(path.read_text())
    assert doc["version"] == 1 and list(doc) == ["version", "config", "opponents"]
    assert doc["config"] == {"opponent_select_alpha": 0.15, "opponent_select_exponent": 2.0}
    assert list(doc["opponents"][0]) == ["checkpoint_name", "checkpoint_step", "win_rate", "avg_swiss_points",
                                         "games_played"]
    assert doc["opponents"][0] == {"checkpoint_name": "step_00001000", "checkpoint_step": 1000, "win_rate": 0.3,
                                   "avg_swiss_points": 2.5, "games_played": 100}
    assert doc["opponents"][1]["games_played"] == 50
    # serde_json's pretty layout: two-space indent, floats keep a fraction
    assert '\n  "version": 1,\n' in path.read_text() and '"opponent_select_exponent": 2.0' in path.read_text()
    q = OpponentPool(2, 0.15, 2.0, 1)
    q.add_checkpoint("step_00001000", 1000, np.ones(3, np.float32))
    cfg = q.load_opponent_stats(path)
    assert cfg == doc["config"]
    assert q.available == p.available
    assert q.models[0] is not None and q.models[1] is None      # the second still needs its model
    q.add_checkpoint("step_00002000", 2000, np.ones(3, np.float32))
    assert q.models[1] is not None and len(q.available) == 2 and q.available[1].win_rate == 0.7
    # a file without avg_swiss_points (#[serde(default)])
    for o in doc["opponents"]:
        del o["avg_swiss_points"]
    path.write_text(json.dumps(doc))
    r = OpponentPool(2, 0.1, 1.0, 1)
    r.load_opponent_stats(path)
    assert [s.avg_swiss_points for s in r.available] == [0.0, 0.0]


def test_add_checkpoint_default_and_duplicate():
    p = _pool([])
    p.add_checkpoint("step_00100000", 100_000, np.zeros(3, np.float32))
    p.add_checkpoint("step_00100000", 100_000, np.ones(3, np.float32))
    assert p.num_available() == 1 and abs(p.available[0].win_rate - 0.5) < EPS and p.available[0].games_played == 0
    assert np.array_equal(p.models[0][0], np.zeros(3, np.float32))
    assert p.get_checkpoint_name(0) == "step_00100000" and p.get_checkpoint_name(3) == "unknown_3"


# ------------------------------------------------ best index / performance ---
def test_get_best_checkpoint_index():
    assert _pool([]).get_best_checkpoint_index() is None
    assert _pool([0.6], swiss=[1.5]).get_best_checkpoint_index() == 0
    assert _pool([0.3, 0.7, 0.5], swiss=[0.8, 2.5, 1.5]).get_best_checkpoint_index() == 1
    # Iterator::max_by keeps the last of equal maxima
    assert _pool([0.5] * 4, swiss=[2.0, 1.0, 2.0, 0.5]).get_best_checkpoint_index() == 2
    assert _pool([0.5] * 3, swiss=[0.0, 0.0, 0.0]).get_best_checkpoint_index() == 2


@pytest.mark.parametrize("win_rates,swiss,players,expected", [
    ([1.0], [3.0], 4, 0.0),               # dominating the best checkpoint
    ([0.0], [0.0], 4, 1.0),               # dominated by it
    ([0.5], [1.5], 4, 0.5),
    ([0.6], [0.6], 2, 0.4),
    ([0.3, 0.1], [2.0, 0.5], 4, 1.0 / 3.0),   # uses the checkpoint with the highest avg_swiss_points
    ([0.5], [4.5], 4, 0.0),               # clamped
])
def test_get_pool_performance(win_rates, swiss, players, expected):
    p = _pool(win_rates, swiss=swiss, games=[100] * len(swiss))
    assert abs(p.get_pool_performance(players) - expected) < 1e-6


def test_get_pool_performance_none():
    assert _pool([]).get_pool_performance(4) is None
    p = _pool([0.5], swiss=[1.5], games=[100])
    assert p.get_pool_performance(1) is None and p.get_pool_performance(0) is None
    assert _pool([0.5], swiss=[1.5], games=[0]).get_pool_performance(4) is None


# ------------------------------------------------- device sums equivalence ---
def _random_completions(rng, n, P, K):
    out = []
    for _ in range(n):
        lp = int(rng.integers(0, P))
        if rng.random() < 0.3:            # ties share a placement (Connect Four draws, Skull)
            placements = [int(x) for x in rng.integers(1, P + 1, P)]
        else:
            placements = [int(x) + 1 for x in rng.permutation(P)]
        p2o = [-1 if p == lp else int(rng.integers(0, K)) for p in range(P)]
        out.append((placements, lp, p2o))
    return out


@pytest.mark.parametrize("P,K", [(2, 3), (4, 5), (6, 15)])
def test_queue_results_equals_game_by_game(P, K):
    rng = np.random.default_rng(P * 100 + K)
    slot_to_pool = [int(x) for x in rng.permutation(K + 4)[:K]]       # device slot -> pool index
    games = _random_completions(rng, 500, P, K)
    a = _pool([0.5] * (K + 4), num_players=P)
    b = _pool([0.5] * (K + 4), num_players=P)
    wins = np.zeros(K, np.int32); cnt = np.zeros(K, np.int32); swiss = np.zeros(K, np.int64)
    for placements, lp, p2o in games:
        a.queue_game_result(placements, lp, [None if m < 0 else slot_to_pool[m] for m in p2o])
        for seat, m in enumerate(p2o):    # the device's sums (opponents.hip k_opp_seats)
            if m >= 0:
                cnt[m] += 1
                swiss[m] += P - placements[lp]
                wins[m] += placements[lp] < placements[seat]
    b.queue_results(wins, cnt, swiss, slot_to_pool)
    assert a.pending_rotation_stats == b.pending_rotation_stats and len(a.pending_rotation_stats) > 1
    a.apply_pending_win_rate_updates(); b.apply_pending_win_rate_updates()
    assert a.available == b.available
    assert sum(s.games_played for s in a.available) == 500 * (P - 1)


def test_queue_game_result_counts():
    p = _pool([0.5, 0.5, 0.5], num_players=4)
    p.queue_game_result([2, 1, 4, 3], 0, [None, 0, 1, 1])     # learner second of four
    assert p.pending_rotation_stats == {0: [0, 1, 2.0], 1: [2, 2, 4.0]}


# ------------------------------------------------------------- the sampler ---
def test_sample_opponent_fallbacks_and_draws():
    assert _pool([]).sample_opponent() is None
    p = _pool([0.2, 0.5])
    pos = p.rng.pos
    assert p.sample_opponent(exclude=[0, 1]) in (0, 1)        # all excluded: gen_range over the pool
    assert p.rng.pos == pos + 2
    p = _pool([1.0, 1.0, 1.0])
    pos = p.rng.pos
    assert p.sample_opponent(exclude=[1]) in (0, 2)           # zero weights: gen_range over the eligible
    assert p.rng.pos == pos + 2
    p = _pool([0.2, 0.5, 1.0])
    pos = p.rng.pos
    assert p.sample_opponent(exclude=[0]) == 1                # the only weight left
    assert p.rng.pos == pos + 2                               # one f64 draw


def test_refresh_current_opponents_unique_and_deterministic():
    a = _pool([0.2, 0.5, 0.8, 0.4, 0.6], num_players=4, seed=9)
    b = _pool([0.2, 0.5, 0.8, 0.4, 0.6], num_players=4, seed=9)
    hist_a, hist_b = [], []
    for _ in range(50):
        a.refresh_current_opponents(); b.refresh_current_opponents()
        hist_a.append(a.sample_all_slots()); hist_b.append(b.sample_all_slots())
        assert len(set(hist_a[-1])) == 3
    assert hist_a == hist_b and len({tuple(h) for h in hist_a}) > 5
    c = _pool([0.2, 0.5, 0.8, 0.4, 0.6], num_players=4, seed=10)
    hist_c = []
    for _ in range(50):
        c.refresh_current_opponents(); hist_c.append(c.sample_all_slots())
    assert hist_c != hist_a
    small = _pool([0.5], num_players=4)         # fewer checkpoints than slots: the fallback repeats it
    small.refresh_current_opponents()
    assert small.current_opponents == [0, 0, 0]


def test_sample_opponent_follows_selection_probabilities():
    """20 000 independent draws: each opponent's count is Binomial(n, p_i), so its frequency
    lies within 5 sigma = 5 sqrt(p_i (1 - p_i) / n) of p_i (a miss has probability < 6e-7 each)"""
    n = 20_000
    for exponent, seed in ((1.0, 42), (2.0, 7)):
        p = _pool([0.2, 0.5, 0.8, 1.0, 0.35], exponent=exponent, seed=seed)
        probs = p.compute_all_selection_probabilities()
        counts = np.zeros(5, np.int64)
        for _ in range(n):
            counts[p.sample_opponent()] += 1
        assert counts[3] == 0                     # win_rate 1: never drawn
        for i, pi in enumerate(probs):
            assert abs(counts[i] / n - pi) <= 5.0 * math.sqrt(pi * (1.0 - pi) / n), (exponent, i, counts, probs)
