"""Python restatement of plackett_luce.rs (the checker of the rating tests): expansion, MM loop,
Fisher information, inversion and Elo conversion, line for line in the reference's order, f64,
math.exp / math.log.  Also the simulated fixtures the rating tests share."""
import math
import random
from dataclasses import dataclass

ELO_SCALE = 400.0 / 2.302585092994046   # 400 / LN_10, plackett_luce.rs:131


@dataclass
class Config:
    max_iterations: int = 100
    convergence_threshold: float = 1e-6
    epsilon: float = 1e-10
    anchor_elo: float = 1000.0
    ci_inflation_factor: float = 1.3


@dataclass
class Result:
    ratings: list          # [(rating, uncertainty)]
    gammas: list
    converged: bool
    iterations_used: int
    final_delta: float
    deltas: list           # max_change of every iteration
    n_comparisons: int = 0


def expand_games_to_comparisons(games, weights=None):
    """:195-254 -> [(winner, losers, weight)]; weights[g] multiplies game g's comparison weights"""
    comparisons = []
    for gi, (players, placements) in enumerate(games):
        if len(players) <= 1:
            continue
        gw = 1.0 if weights is None else weights[gi]
        groups = {}
        for local_idx, placement in enumerate(placements):
            groups.setdefault(placement, []).append(players[local_idx])
        sorted_placements = sorted(groups)
        for pos_idx, current in enumerate(sorted_placements):
            current_players = groups[current]
            lower = []
            for later in sorted_placements[pos_idx + 1:]:
                lower.extend(groups[later])
            if not lower:
                continue
            weight = (1.0 / float(len(current_players))) * gw
            for tied in current_players:
                comparisons.append((tied, list(lower), weight))
    return comparisons


def count_games_per_player(games, num_players):
    counts = [0] * num_players
    for players, _ in games:
        for p in players:
            if p < num_players:
                counts[p] += 1
    return counts


def mm_update(comparisons, gammas, num_players, epsilon):
    """:271-316"""
    wins = [0.0] * num_players
    denom = [0.0] * num_players
    for winner, losers, weight in comparisons:
        wins[winner] += weight
        participants = [winner] + losers
        sum_exp = 0.0
        for p in participants:
            sum_exp += math.exp(gammas[p])
        if sum_exp > epsilon:
            contribution = weight / sum_exp
            for p in participants:
                denom[p] += contribution
    new = [0.0] * num_players
    for i in range(num_players):
        if wins[i] > epsilon and denom[i] > epsilon:
            new[i] = math.log(wins[i] / denom[i])
        elif denom[i] > epsilon:
            new[i] = gammas[i] - 1.0
        else:
            new[i] = gammas[i]
    return new


def softmax(logits):
    """:168-180"""
    mx = -math.inf
    for x in logits:
        mx = max(mx, x)
    e = [math.exp(x - mx) for x in logits]
    s = 0.0
    for x in e:
        s += x
    if s == 0.0:
        return [1.0 / len(logits)] * len(logits)
    return [x / s for x in e]


def compute_hessian(comparisons, gammas, num_players):
    """:320-353"""
    h = [[0.0] * num_players for _ in range(num_players)]
    for winner, losers, weight in comparisons:
        participants = [winner] + losers
        probs = softmax([gammas[p] for p in participants])
        for li, pi in enumerate(participants):
            for lj, pj in enumerate(participants):
                if li == lj:
                    h[pi][pj] += weight * probs[li] * (1.0 - probs[li])
                else:
                    h[pi][pj] -= weight * probs[li] * probs[lj]
    return h


def invert_matrix(matrix, epsilon):
    """:361-425"""
    n = len(matrix)
    if n == 0:
        return []
    aug = [list(row) + [0.0] * n for row in matrix]
    for i in range(n):
        aug[i][n + i] = 1.0
    for col in range(n):
        max_row, max_val = col, abs(aug[col][col])
        for row in range(col + 1, n):
            if abs(aug[row][col]) > max_val:
                max_val, max_row = abs(aug[row][col]), row
        aug[col], aug[max_row] = aug[max_row], aug[col]
        if abs(aug[col][col]) < epsilon:
            return [[100.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
        pivot = aug[col][col]
        pr = aug[col]
        for j in range(2 * n):
            pr[j] /= pivot
        for row in range(n):
            if row != col:
                rr = aug[row]
                factor = rr[col]
                for j in range(2 * n):
                    rr[j] -= factor * pr[j]
    return [row[n:] for row in aug]


def compute_ratings(num_players, games, anchor, config=None, weights=None):
    """:437-614"""
    cfg = config or Config()
    default = [(cfg.anchor_elo, 350.0)] * num_players
    if num_players == 0:
        return Result([], [], True, 0, 0.0, [])
    if not games:
        return Result(default, [0.0] * num_players, True, 0, 0.0, [])
    games_played = count_games_per_player(games, num_players)
    comparisons = expand_games_to_comparisons(games, weights)
    if not comparisons:
        return Result(default, [0.0] * num_players, True, 0, 0.0, [])
    gammas = [0.0] * num_players
    iterations_used, final_delta, converged, deltas = 0, 1.7976931348623157e308, False, []
    for iteration in range(cfg.max_iterations):
        iterations_used = iteration + 1
        new = mm_update(comparisons, gammas, num_players, cfg.epsilon)
        s = 0.0
        for g in new:
            s += g
        mean = s / float(num_players)
        centered = [g - mean for g in new]
        max_change = 0.0
        for old, c in zip(gammas, centered):
            d = abs(old - c)
            if d > max_change:          # f64::max: a NaN is ignored
                max_change = d
        final_delta = max_change
        deltas.append(max_change)
        gammas = centered
        if max_change < cfg.convergence_threshold:
            converged = True
            break
        if any(not math.isfinite(g) for g in gammas):
            gammas = [0.0] * num_players
            break
    hessian = compute_hessian(comparisons, gammas, num_players)
    active = [i for i in range(num_players) if games_played[i] > 0 and i != anchor]
    reduced = [[hessian[i][j] for j in active] for i in active]
    for ri in range(len(active)):
        reduced[ri][ri] += 1e-6
    cov = invert_matrix(reduced, cfg.epsilon)
    unc = [2.0] * num_players
    unc[anchor] = 0.0
    for ri, i in enumerate(active):
        if cov[ri][ri] > 0.0:
            unc[i] = math.sqrt(cov[ri][ri])
    shift = (cfg.anchor_elo - 1500.0) / ELO_SCALE - gammas[anchor]
    ratings = []
    for i in range(num_players):
        if games_played[i] > 0:
            ratings.append((1500.0 + ELO_SCALE * (gammas[i] + shift), (ELO_SCALE * unc[i]) * cfg.ci_inflation_factor))
        else:
            ratings.append((cfg.anchor_elo, 350.0))
    return Result(ratings, gammas, converged, iterations_used, final_delta, deltas, len(comparisons))


# ------------------------------------------------------------------- fixtures ---
def simulate(seed, num_players, sizes, n_games, tie_prob=0.1):
    """players with Gaussian log-strengths; finishing orders drawn from the Plackett-Luce model;
    each finisher ties with the one before with probability tie_prob -> [(players, placements)]"""
    rng = random.Random(seed)
    strength = [math.exp(rng.gauss(0.0, 1.0)) for _ in range(num_players)]
    games = []
    for _ in range(n_games):
        k = min(rng.choice(sizes), num_players)
        seats = rng.sample(range(num_players), k)
        left, order = list(seats), []
        while left:
            tot = sum(strength[p] for p in left)
            x, acc, pick = rng.random() * tot, 0.0, left[-1]
            for p in left:
                acc += strength[p]
                if x < acc:
                    pick = p
                    break
            left.remove(pick)
            order.append(pick)
        place, placement_of = 1, {}
        for pos, p in enumerate(order):
            if pos > 0 and rng.random() >= tie_prob:
                place = pos + 1
            placement_of[p] = place
        games.append((seats, [placement_of[p] for p in seats]))
    return games


# name -> (seed, players, game sizes, games); the anchor is the last player
SIMULATED = {
    "A": (11, 2, (2,), 30),
    "M": (12, 7, (2, 3, 4, 5, 6), 400),
    "six": (13, 12, (6,), 600),
    "D": (14, 40, (4,), 3000),
    "N130": (15, 130, (4,), 4000),
    # few players, long incidence lists (about 1,660 entries each): past the 1,024 entries from
    # which the device cuts a player's list into pieces summed apart
    "long": (16, 3, (3,), 1000),
}

# by hand: 9 players; games of 1, 2, 3 and 6 players; a three-way tie for first; a tie for last;
# player 7 has no games; player 8 never wins; the anchor (4) sits in the middle
EDGE_PLAYERS, EDGE_ANCHOR = 9, 4
EDGE_GAMES = [
    ([0], [1]),
    ([0, 1], [1, 2]),
    ([1, 2], [1, 2]),
    ([2, 0], [1, 2]),
    ([3, 4, 5], [1, 1, 1]),
    ([3, 4, 5], [2, 1, 3]),
    ([5, 3, 4], [1, 2, 2]),
    ([0, 1, 2, 3, 4, 5], [1, 1, 1, 4, 5, 6]),
    ([5, 4, 3, 2, 1, 0], [1, 2, 3, 4, 5, 5]),
    ([6, 0, 8], [2, 1, 3]),
    ([6, 8], [1, 2]),
    ([4, 6, 8], [2, 1, 3]),
    ([1, 6], [2, 1]),
    ([3, 0], [1, 2]),
    ([4, 1, 8, 6, 2, 5], [3, 2, 6, 1, 4, 4]),
    ([2, 4], [2, 1]),
    ([6, 3], [2, 1]),
]

_cache = {}


def fixture(name):
    """-> (num_players, games, anchor)"""
    if name == "edge":
        return EDGE_PLAYERS, EDGE_GAMES, EDGE_ANCHOR
    if name not in _cache:
        seed, n, sizes, g = SIMULATED[name]
        _cache[name] = simulate(seed, n, sizes, g)
    return SIMULATED[name][1], _cache[name], SIMULATED[name][1] - 1


FIXTURES = ("A", "M", "six", "D", "N130", "long", "edge")

_ref_cache = {}


def reference(name):
    """the restatement's result on a fixture, computed once"""
    if name not in _ref_cache:
        n, games, anchor = fixture(name)
        _ref_cache[name] = compute_ratings(n, games, anchor)
    return _ref_cache[name]


_spread_cache = {}


def order_spread(name, orderings=8):
    """the largest spread of the restatement's own outputs over random orderings of the same
    games (the identity included): {"rating", "uncertainty", "final_delta", "gamma"}"""
    if name in _spread_cache:
        return _spread_cache[name]
    n, games, anchor = fixture(name)
    runs = [reference(name)]
    rng = random.Random(1000 + len(games))
    for _ in range(orderings):
        g = list(games)
        rng.shuffle(g)
        runs.append(compute_ratings(n, g, anchor))
    def spread(f):
        vals = [f(r) for r in runs]
        return max(max(v[i] for v in vals) - min(v[i] for v in vals) for i in range(len(vals[0]))) if vals[0] else 0.0
    out = {"rating": spread(lambda r: [x[0] for x in r.ratings]),
           "uncertainty": spread(lambda r: [x[1] for x in r.ratings]),
           "gamma": spread(lambda r: r.gammas),
           "final_delta": spread(lambda r: [r.final_delta]),
           "iterations": sorted(set(r.iterations_used for r in runs))}
    _spread_cache[name] = out
    return out
