"""A round-robin round of evaluation pods: one bppo_evaluate_pods loop against the pods one
after another.

    python scripts/eval_pods_timing.py [--models 8 --envs 64 --games 256 --repeats 7] [--only pods]

Connect Four, the configs/connect_four.toml MLP (2 x 512), `models` distinct checkpoints, all
C(models, 2) pods, `envs` envs and `games` games per pod, the env's default temperature
schedule, pod k seeded with seed + k on every path (so the three play the same games).
Timed after one warm-up each, `repeats` times, medians with min and max:
    pods            bppo.evaluate_pods: one context, one loop for all pods
    sequential      one bppo.evaluate call per pod (a context per pod, as the public surface
                    of the parent commit plays a round)
    sequential_ctx  bppo_evaluate per pod on one reused context of `envs` envs
Prints one JSON line.  --only pods runs the first path alone, once after the warm-up (for a
kernel trace).  Reported, not gated."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "burn-ppo_amd"))


def _timed(fn, repeats):
    fn()                                                    # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return ts, out


def _summary(ts, games):
    med = statistics.median(ts)
    return {"median_s": round(med, 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4),
            "games_per_sec": round(games / med, 1)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", type=int, default=8)
    p.add_argument("--envs", type=int, default=64)
    p.add_argument("--games", type=int, default=256)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--only", choices=["pods"], default=None)
    a = p.parse_args()
    import numpy as np
    import torch
    import bppo
    from bppo.eval import evaluate_ctx
    torch.cuda.set_device(0)
    cfg = bppo.make_config("connect_four", num_envs=a.envs, num_steps=8, num_minibatches=1, num_epochs=1)
    params = [(bppo.orthogonal_init(cfg, seed=s + 1) * np.float32(3.0)).astype(np.float32) for s in range(a.models)]
    sched = bppo.TempSchedule.env_default("connect_four")
    pods = bppo.round_robin_pods(a.models, 2)
    seeds = [a.seed + k for k in range(len(pods))]
    total = len(pods) * a.games
    out = {"workload": "eval pods connect_four mlp 2x512", "models": a.models, "pods": len(pods),
           "envs_per_pod": a.envs, "games_per_pod": a.games, "repeats": a.repeats}

    def run_pods():
        return bppo.evaluate_pods(cfg, params, None, pods, a.games, a.envs, sched, seeds=seeds)

    def run_sequential():
        return [bppo.evaluate(cfg, [params[i], params[j]], None, [0, 1], a.games, sched, seeds[k])
                for k, (i, j) in enumerate(pods)]

    ts, stats = _timed(run_pods, 1 if a.only else a.repeats)
    out["pods"] = _summary(ts, total)
    out["pods"]["loop_steps"] = max(g[2] for st in stats for g in st.games) + 1
    if not a.only:
        ts, seq = _timed(run_sequential, a.repeats)
        out["sequential"] = _summary(ts, total)
        out["sequential"]["loop_steps"] = sum(max(g[2] for g in st.games) + 1 for st in seq)
        out["same_games"] = all(x.games == y.games and x.game_outcomes == y.game_outcomes and
                                x.rng_word_pos == y.rng_word_pos for x, y in zip(stats, seq))
        ctx = bppo.Context(cfg, device=0)
        try:
            ts, _ = _timed(lambda: [evaluate_ctx(ctx, [params[i], params[j]], None, [0, 1], a.games, sched, seeds[k])
                                    for k, (i, j) in enumerate(pods)], a.repeats)
        finally:
            ctx.close()
        out["sequential_ctx"] = _summary(ts, total)
        out["speedup_vs_sequential"] = round(out["sequential"]["median_s"] / out["pods"]["median_s"], 2)
        out["speedup_vs_sequential_ctx"] = round(out["sequential_ctx"]["median_s"] / out["pods"]["median_s"], 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
