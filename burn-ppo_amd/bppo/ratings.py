"""Plackett-Luce ratings (plackett_luce.rs) over the device rating table (bppo_ratings_*).

    RatingTable       the table: games and their comparisons stay in device memory; fit() iterates
    compute_ratings   plackett_luce.rs:437-614, one shot
    PlackettLuceConfig / PlayerRating / RatingStats / RatingResult   the reference's structs

backend="device" runs the fit's kernels (bit-reproducible: no floating-point atomics);
backend="host" is the reference's arithmetic in the reference's order and needs no GPU
(RatingTable(device=None))."""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L

BACKENDS = {"device": 0, "host": 1}


@dataclass
class PlackettLuceConfig:
    """plackett_luce.rs:102-127"""
    max_iterations: int = 100
    convergence_threshold: float = 1e-6
    epsilon: float = 1e-10
    anchor_elo: float = 1000.0
    ci_inflation_factor: float = 1.3


@dataclass
class PlayerRating:
    """plackett_luce.rs:50-76"""
    rating: float = 1000.0
    uncertainty: float = 350.0

    def confidence_interval(self):
        """95% bounds (plackett_luce.rs:61-66)"""
        return (self.rating - 2.0 * self.uncertainty, self.rating + 2.0 * self.uncertainty)


@dataclass
class RatingStats:
    """plackett_luce.rs:80-89, and the size of the fitted table"""
    converged: bool = True
    iterations_used: int = 0
    final_delta: float = 0.0
    computation_time_ms: float = 0.0
    n_games: int = 0
    n_comparisons: int = 0


@dataclass
class RatingResult:
    ratings: list = field(default_factory=list)
    stats: RatingStats = field(default_factory=RatingStats)
    gammas: np.ndarray = None      # centred log-strengths before the anchor shift


def pad_games(players, placements):
    """ragged lists (or padded arrays) -> int32 [n][P] arrays, -1 / 0 past a game's end"""
    if isinstance(players, np.ndarray) and isinstance(placements, np.ndarray):
        pl, pc = np.ascontiguousarray(players, np.int32), np.ascontiguousarray(placements, np.int32)
        if pl.ndim != 2 or pl.shape != pc.shape:
            raise ValueError("add_games: players and placements are [n][P] arrays of one shape")
        return pl, pc
    n = len(players)
    if len(placements) != n:
        raise ValueError("add_games: players and placements list different numbers of games")
    P = max([len(g) for g in players] + [1])
    pl, pc = np.full((n, P), -1, np.int32), np.zeros((n, P), np.int32)
    for g, (a, b) in enumerate(zip(players, placements)):
        if len(a) != len(b):
            raise ValueError("players and placements must have same length")
        pl[g, :len(a)] = a
        pc[g, :len(b)] = b
    return pl, pc


class RatingTable:
    """bppo_ratings: device=None makes a host-only table (backend "host" only)."""

    def __init__(self, device=0, stream=None):
        self.h = None
        self.device = device
        h = C.c_void_p()
        st = L.lib().bppo_ratings_create(-1 if device is None else int(device), stream, C.byref(h))
        self.h = h
        if st != L.OK:
            msg = L.lib().bppo_ratings_last_error(h).decode() if h else ""
            self.close()
            raise L.BppoError(st, msg)

    def _check(self, st):
        if st != L.OK:
            raise L.BppoError(st, L.lib().bppo_ratings_last_error(self.h).decode())

    def close(self):
        if self.h:
            L.lib().bppo_ratings_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def clear(self):
        self._check(L.lib().bppo_ratings_clear(self.h))

    @property
    def num_games(self):
        n = C.c_int64()
        self._check(L.lib().bppo_ratings_num_games(self.h, C.byref(n)))
        return n.value

    def last_fit_phases(self):
        """wall ms of the last fit: {incidence list, MM iterations, Fisher information, host inversion}"""
        ms = np.zeros(4, np.float64)
        self._check(L.lib().bppo_ratings_last_fit_phases(self.h, L.ptr(ms)))
        return dict(zip(("incidence_ms", "iterations_ms", "fisher_ms", "inversion_ms"), ms.tolist()))

    def add_games(self, players, placements, weight=None):
        """players / placements: ragged lists of games, or [n][P] arrays padded with -1;
        weight [n]: a game with weight w counts as w identical games"""
        pl, pc = pad_games(players, placements)
        if pl.shape[0] == 0:
            return
        w = None if weight is None else np.ascontiguousarray(weight, np.float64).reshape(-1)
        if w is not None and w.size != pl.shape[0]:
            raise ValueError("add_games: one weight per game")
        self._check(L.lib().bppo_ratings_add_games(self.h, pl.shape[0], pl.shape[1], L.ptr(pl), L.ptr(pc), L.ptr(w)))

    def add_completions(self, ctx, learner_player, slot_to_player):
        """the kept opponent completions of ctx's last rollout, on the device (main.rs:755-790);
        slot_to_player[k] = player id of device model slot k.  -> games appended"""
        s2p = np.ascontiguousarray(slot_to_player, np.int32).reshape(-1)
        added = C.c_int64()
        self._check(L.lib().bppo_ratings_add_completions(self.h, ctx.h, int(learner_player), L.ptr(s2p), s2p.size,
                                                         C.byref(added)))
        return added.value

    def fit(self, num_players, anchor, config=None, backend="device"):
        cfg = config or PlackettLuceConfig()
        c = L.PlConfig(int(cfg.max_iterations), BACKENDS[backend], float(cfg.convergence_threshold),
                       float(cfg.epsilon), float(cfg.anchor_elo), float(cfg.ci_inflation_factor))
        n = int(num_players)
        rating, unc, gam = (np.zeros(max(n, 1), np.float64) for _ in range(3))
        st = L.PlStats()
        self._check(L.lib().bppo_ratings_fit(self.h, C.byref(c), n, int(anchor), L.ptr(rating), L.ptr(unc), L.ptr(gam),
                                             C.byref(st)))
        return RatingResult([PlayerRating(float(rating[i]), float(unc[i])) for i in range(n)],
                            RatingStats(bool(st.converged), st.iterations_used, st.final_delta, st.fit_ms, st.n_games,
                                        st.n_comparisons), gam[:n].copy())


def compute_ratings(num_players, games, anchor, config=None, device=0, backend=None):
    """plackett_luce.rs:437-614: games = [(players, placements), ...]; device=None fits on the
    host (the reference's arithmetic)"""
    with RatingTable(device=device) as t:
        t.add_games([g[0] for g in games], [g[1] for g in games])
        return t.fit(num_players, anchor, config, backend or ("host" if device is None else "device"))
