"""Throughput of device-side evaluation matches (bppo_evaluate).

    python scripts/bench_eval.py [--num-envs 4096 --games 20000 --repeats 3] [--cpu]

Connect Four, the configs/connect_four.toml MLP (2 x 512), two distinct models, the
env's default temperature schedule (0.4 -> 0.0 at move 10).  Prints one JSON line:
games/s and env-steps/s (the moves of the recorded games) of the best of `repeats`
calls after one warm-up call.  --cpu times the Python restatement of the reference's
loop on the CPU oracle's primitives (tests/eval_ref.py) on the same settings instead;
it is a parity checker, not an optimized CPU path.  Reported, not gated."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "burn-ppo_amd"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--num-envs", type=int, default=4096)
    p.add_argument("--games", type=int, default=20000)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--cpu", action="store_true", help="time tests/eval_ref.py (oracle primitives) instead")
    a = p.parse_args()
    import numpy as np
    import bppo
    cfg = bppo.make_config("connect_four", num_envs=a.num_envs, num_steps=8, num_minibatches=1, num_epochs=1)
    params = [(bppo.orthogonal_init(cfg, seed=s) * np.float32(3.0)).astype(np.float32) for s in (1, 2)]
    sched = bppo.TempSchedule.env_default("connect_four")
    out = {"workload": "eval connect_four mlp 2x512", "num_envs": a.num_envs, "num_games": a.games}
    if a.cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import eval_ref as R
        d = R.O.mlp_desc(86, 7, cfg["hidden_size"], cfg["num_hidden"])
        models = [R.Model(d, q) for q in params]
        t0 = time.perf_counter()
        ref = R.run_stats_mode("connect_four", a.num_envs, 2, models, [0, 1], a.games,
                               R.TempSchedule(sched.initial, sched.final_temp, sched.cutoff, sched.decay), a.seed)
        dt = time.perf_counter() - t0
        moves, steps, games = sum(g[2] for g in ref["games"]), ref["steps"], len(ref["games"])
        out["path"] = "python restatement on the CPU oracle"
    else:
        import torch
        from bppo.eval import evaluate_ctx
        torch.cuda.set_device(0)
        ctx = bppo.Context(cfg, device=0)
        evaluate_ctx(ctx, params, None, [0, 1], min(a.games, 2 * a.num_envs), sched, a.seed)     # warm-up
        dt = float("inf")
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            rec, pos = evaluate_ctx(ctx, params, None, [0, 1], a.games, sched, a.seed)
            dt = min(dt, time.perf_counter() - t0)
        ctx.close()
        moves, steps, games = int(rec["length"].sum()), int(rec["step"].max()) + 1, len(rec)
        out["path"] = "device"
        out["rng_word_pos"] = int(pos)
    out.update({"games": games, "loop_steps": steps, "seconds": round(dt, 4), "games_per_sec": round(games / dt, 1),
                "env_steps_per_sec": round(moves / dt, 1), "ms_per_loop_step": round(dt / steps * 1000, 4)})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
