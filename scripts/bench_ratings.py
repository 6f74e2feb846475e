"""Plackett-Luce fits on the device rating table against the host backend.

    python scripts/bench_ratings.py [--repeats 5] [--games 10000 100000 1000000] [--players 64 512]
                                    [--no-host] [--inversion]

Simulated four-player tables: Gaussian log-strengths, finishing orders drawn from the
Plackett-Luce model (Gumbel-max), each finisher tied with the one before with probability 0.1,
anchor = the last player.  Per table: the append (host arrays -> device games + comparisons), then
fits on one table after one warm-up, `repeats` times: median (min - max) ms per fit, iterations,
us per iteration (the MM loop alone), the share of the fit spent in the host inversion, and the
incidence-list build of the first fit.  Backend 0 (device) against backend 1 (host: the
reference's arithmetic in its order, which stands in for the reference).  Every timed call ends
in a host read of its results, so the times are wall times of finished work.  Repeated fits must
return identical bits.  One JSON line per run.  --inversion: the host inversion alone at 128 and
1,024 players (a 127 x 127 and a 1,023 x 1,023 matrix).  Reported, not gated."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "burn-ppo_amd"))


def simulate(np, seed, players, games, size=4, tie_prob=0.1):
    rng = np.random.default_rng(seed)
    strength = rng.normal(0.0, 1.0, players)
    seats = rng.integers(0, players, (games, size)).astype(np.int32)
    while True:                                                    # redraw the games that seat a player twice
        s = np.sort(seats, axis=1)
        dup = np.flatnonzero((s[:, 1:] == s[:, :-1]).any(axis=1))
        if dup.size == 0:
            break
        seats[dup] = rng.integers(0, players, (dup.size, size))
    key = strength[seats] + rng.gumbel(size=(games, size))
    order = np.argsort(-key, axis=1)                               # finishing order, as seat indices
    new_place = rng.random((games, size)) >= tie_prob
    new_place[:, 0] = True
    place_by_rank = np.maximum.accumulate(np.where(new_place, np.arange(1, size + 1), 0), axis=1)
    placements = np.empty((games, size), np.int32)
    np.put_along_axis(placements, order, place_by_rank.astype(np.int32), axis=1)
    return seats, placements


def _fmt(ts):
    return "%.2f (%.2f - %.2f)" % (statistics.median(ts), min(ts), max(ts))


def bench(np, table, n, backend, repeats):
    def run():
        t0 = time.perf_counter()
        r = table.fit(n, n - 1, backend=backend)
        return 1e3 * (time.perf_counter() - t0), r, table.last_fit_phases()
    _, first, ph0 = run()                                          # warm-up: builds the incidence list
    ts, it_ms, inv_ms, same = [], [], [], True
    for _ in range(repeats):
        ms, r, ph = run()
        ts.append(ms)
        it_ms.append(ph["iterations_ms"])
        inv_ms.append(ph["inversion_ms"])
        same = same and r.gammas.tobytes() == first.gammas.tobytes() and \
            [x.uncertainty for x in r.ratings] == [x.uncertainty for x in first.ratings]
    med = statistics.median(ts)
    return {"ms_per_fit": _fmt(ts), "iterations": first.stats.iterations_used, "converged": first.stats.converged,
            "us_per_iteration": round(1e3 * statistics.median(it_ms) / max(first.stats.iterations_used, 1), 1),
            "fisher_ms": round(ph["fisher_ms"], 2), "inversion_ms": round(statistics.median(inv_ms), 2),
            "inversion_share": round(statistics.median(inv_ms) / med, 3),
            "first_fit_incidence_ms": round(ph0["incidence_ms"], 2), "identical_bits": same}, first


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--games", type=int, nargs="+", default=[10**4, 10**5, 10**6])
    p.add_argument("--players", type=int, nargs="+", default=[64, 512])
    p.add_argument("--no-host", action="store_true")
    p.add_argument("--inversion", action="store_true")
    a = p.parse_args()
    import numpy as np
    import torch
    from bppo.ratings import RatingTable
    torch.cuda.set_device(0)
    cases = [(g, n) for n in a.players for g in a.games]
    if a.inversion:
        cases = [(10**5, 128), (10**5, 1024)]
    for games, n in cases:
        pl, pc = simulate(np, 7 + n, n, games)
        with RatingTable(device=0) as t:
            t.add_games(pl[:16], pc[:16])                          # warm-up of the append path
            t.clear()
            t0 = time.perf_counter()
            t.add_games(pl, pc)
            append_ms = 1e3 * (time.perf_counter() - t0)
            row = {"games": games, "players": n, "append_ms": round(append_ms, 2)}
            dev, rd = bench(np, t, n, "device", a.repeats)
            print(json.dumps(dict(row, backend="device", comparisons=rd.stats.n_comparisons, **dev)), flush=True)
            if not a.no_host and not a.inversion:
                host, rh = bench(np, t, n, "host", a.repeats)
                diff = max(abs(x.rating - y.rating) for x, y in zip(rd.ratings, rh.ratings))
                print(json.dumps(dict(row, backend="host", **host, max_rating_diff_vs_device=diff,
                                      same_iterations=rd.stats.iterations_used == rh.stats.iterations_used)), flush=True)


if __name__ == "__main__":
    main()
