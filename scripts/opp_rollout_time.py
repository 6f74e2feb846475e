#!/usr/bin/env python3
"""Device time of an opponent-pool rollout (bppo_last_kernel_ms "rollout"): Connect Four,
K random-initialised opponents, over repeated rollouts of one context.  One JSON line:
median / min / max in ms and the finished opponent games of the last rollout (when the
library reports them).  BPPO_LIB_PATH picks the library, so two builds are compared by
running this once per build, alternating.

    python scripts/opp_rollout_time.py [--num-envs 4096] [--num-steps 128] [--opponents 3]
                                       [--opponent-frac 0.5] [--rollouts 15] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "burn-ppo_amd"))
import bppo  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--num-envs", type=int, default=4096)
    p.add_argument("--num-steps", type=int, default=128)
    p.add_argument("--opponents", type=int, default=3)
    p.add_argument("--opponent-frac", type=float, default=0.5)
    p.add_argument("--rollouts", type=int, default=15)
    p.add_argument("--warmup", type=int, default=3)
    a = p.parse_args()
    cfg = bppo.make_config("connect_four", num_envs=a.num_envs, num_steps=a.num_steps)
    tr = bppo.Trainer(cfg, params=bppo.orthogonal_init(cfg, seed=5))
    P, K = tr.ctx.seats, a.opponents
    n_opp = int(a.num_envs * a.opponent_frac)
    rng = np.random.default_rng(1)
    opp = np.stack([bppo.orthogonal_init(cfg, seed=50 + k) for k in range(K)])
    lp = rng.integers(0, P, n_opp).astype(np.int32)
    po = np.where(np.arange(P)[None, :] == lp[:, None], -1, rng.integers(0, K, (n_opp, P))).astype(np.int32)
    tr.ctx.set_opponents(opp, None, n_opp, lp, po, rng.integers(0, K, P - 1))
    ms = []
    for i in range(a.warmup + a.rollouts):
        bppo.collect_rollouts(tr.ctx)
        if i >= a.warmup:
            ms.append(tr.ctx.kernel_ms("rollout"))
    games = None
    if hasattr(tr.ctx, "opponent_results"):
        games = int(tr.ctx.opponent_results()[1].sum())
    print(json.dumps({"lib": os.path.basename(bppo._lib.LIB_PATH), "num_envs": a.num_envs, "num_steps": a.num_steps,
                      "opponents": K, "opponent_envs": n_opp, "rollouts": len(ms),
                      "rollout_ms_median": round(statistics.median(ms), 3), "rollout_ms_min": round(min(ms), 3),
                      "rollout_ms_max": round(max(ms), 3), "opponent_games_last_rollout": games}))
    tr.close()


if __name__ == "__main__":
    main()
