"""What the device episode statistics cost the pipelined loop.

    python scripts/bench_episode_stats.py [--steps 10] [--repeats 5] [--warmup 3] [--configs cfgb c4]

Per config one trainer, warmed up, then `repeats` pairs of timed Trainer.train_updates(steps)
calls, alternating bppo_set_episode_stats off and on in the same process (off first in even
pairs, on first in odd ones, so a drift over the run lands on both sides).  The on side
includes reading every rollout's block into the EpisodeWindow.  Each timed call ends with the
stream drained, so the times are wall times of finished work.  Reports ms per update: median
(min - max) of either side, their difference, and the off side's own spread to judge it by.
One JSON line per config.  Reported, not gated.

    cfgb  bench.py's workload: CartPole, num_envs 65536, num_steps 128, the fused 2 x 64 net
    c4    Connect Four, num_envs 4096, num_steps 128, MLP 2 x 256

--off-only: only the off side (a kernel trace of it is compared with the parent commit's).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "burn-ppo_amd"))

CONFIGS = {
    "cfgb": ("cartpole", dict(num_envs=65536, num_steps=128)),
    "c4": ("connect_four", dict(num_envs=4096, num_steps=128, hidden_size=256, num_hidden=2)),
}


def _fmt(ts):
    return "%.3f (%.3f - %.3f)" % (statistics.median(ts), min(ts), max(ts))


def run(bppo, name, steps, repeats, warmup, off_only):
    from bppo.episodes import EpisodeWindow, set_episode_stats
    preset, over = CONFIGS[name]
    cfg = bppo.make_config(preset, **over)
    tr = bppo.Trainer(cfg, init_seed=0)
    window = EpisodeWindow(tr.ctx.seats)

    def timed(on):
        set_episode_stats(tr.ctx, on)
        tr.episodes = window if on else None
        window.clear()
        t0 = time.perf_counter()
        mets, _ = tr.train_updates(steps)
        dt = time.perf_counter() - t0
        return 1e3 * dt / steps, sum(m["episodes"] for m in mets), window.episodes

    tr.train_updates(warmup)
    if not off_only:
        timed(True)                                   # the statistics' scratch is allocated here
    off, on, episodes = [], [], 0
    for r in range(repeats):
        order = (False,) if off_only else ((False, True) if r % 2 == 0 else (True, False))
        for side in order:
            ms, n_eps, n_win = timed(side)
            (on if side else off).append(ms)
            episodes = n_eps
            if side:
                assert n_win == n_eps, (n_win, n_eps)  # the window saw every rollout of the call
    out = {"config": name, "num_envs": cfg["num_envs"], "num_steps": cfg["num_steps"], "steps_per_call": steps,
           "repeats": repeats, "episodes_per_call": episodes, "off_ms_per_update": _fmt(off),
           "off_spread_ms": round(max(off) - min(off), 3)}
    if on:
        out["on_ms_per_update"] = _fmt(on)
        out["on_minus_off_median_ms"] = round(statistics.median(on) - statistics.median(off), 3)
    tr.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    p.add_argument("--off-only", action="store_true")
    a = p.parse_args()
    import bppo
    for name in a.configs:
        print(json.dumps(run(bppo, name, a.steps, a.repeats, a.warmup, a.off_only)), flush=True)


if __name__ == "__main__":
    main()
