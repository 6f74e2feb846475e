"""CartPole checkpoint evaluation on the device: bppo_evaluate_episodes.

    python scripts/bench_eval_cartpole.py [--repeats 5] [--steps-per-launch 0] [--only one_pod_balance]
                                          [--hidden 64 --layers 2]
    python scripts/bench_eval_cartpole.py --cpu

The 64 x 2 relu net of configs/cartpole.toml (--hidden / --layers: another fused shape), the trait's default temperature (0.3), two nets:
the balancing controller (episodes run to the 500-step truncation) and an orthogonal-init
random net (episodes of a few dozen steps).  Workloads:
    one_pod_*    one pod of 1,024 envs, 10,000 episodes: one thread block, one CU
    pods_*       256 pods x 256 envs, 1,000 episodes each: a block on every CU
Each is timed on one reused context after one warm-up, `repeats` times: median (min - max) ms,
loop iterations, us per iteration, episodes/s and recorded env-steps/s (the lengths of the
recorded episodes over the time); repeated calls must play identical games.  One JSON line per
workload.  --only runs one workload alone (with --repeats 1: for a kernel trace).
--cpu: the Python restatement (tests/eval_ref_cartpole.py) on a reduced size.  It is the parity
checker, not a baseline: an interpreter loop over ctypes calls.  Reported, not gated."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "burn-ppo_amd"))

BALANCE_C, BALANCE_K = (0.1, 0.5, 10.0, 2.0, 0.0), 4.0


def balance_net(n_params, H, NL):
    """push right iff c . obs >= 0: hidden units 0 and 1 carry +-(c . obs) through both relu
    layers, logits = -+K (h0 - h1)"""
    import numpy as np
    p = np.zeros(n_params, np.float32)
    w0 = p[:5 * H].reshape(5, H)
    w0[:, 0] = BALANCE_C
    w0[:, 1] = [-c for c in BALANCE_C]
    off = 5 * H + H
    if NL == 2:
        w1 = p[off:off + H * H].reshape(H, H)
        w1[0, 0] = w1[1, 1] = 1.0
        off += H * H + H
    wp = p[off:off + 2 * H].reshape(H, 2)
    wp[0] = [-BALANCE_K, BALANCE_K]
    wp[1] = [BALANCE_K, -BALANCE_K]
    return p


def _fmt(ts):
    return "%.1f (%.1f - %.1f)" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--steps-per-launch", type=int, default=0)
    p.add_argument("--only", default=None)
    p.add_argument("--cpu", action="store_true")
    p.add_argument("--hidden", type=int, default=64, choices=(16, 32, 64))
    p.add_argument("--layers", type=int, default=2, choices=(1, 2))
    a = p.parse_args()
    H, NL = a.hidden, a.layers
    import numpy as np
    import bppo
    cfg = bppo.make_config("cartpole", hidden_size=H, num_hidden=NL, activation="relu", num_envs=8, num_steps=4,
                           num_minibatches=1, num_epochs=1)
    rnd = (bppo.orthogonal_init(cfg, seed=1) * np.float32(3.0)).astype(np.float32)
    nets = {"balance": balance_net(rnd.size, H, NL), "random": rnd}
    sched = bppo.TempSchedule.env_default("cartpole")

    if a.cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import eval_ref_cartpole as X
        for name, E, games in (("balance", 16, 32), ("random", 128, 512)):
            t0 = time.perf_counter()
            out = X.run_reference(X.O.mlp_desc(5, 2, H, NL, relu=True), nets[name], None, E, games,
                                  (0.3, 0.0, None, False), 1, 100000)
            dt = time.perf_counter() - t0
            steps = sum(g[2] for g in out["games"])
            print(json.dumps({"workload": "parity checker (Python restatement), not a baseline", "net": name,
                              "envs": E, "episodes": games, "s": round(dt, 2), "loop_steps": out["steps"],
                              "episodes_per_sec": round(games / dt, 1), "env_steps_per_sec": round(steps / dt, 1)}),
                  flush=True)
        return

    import torch
    from bppo.eval import evaluate_episodes_ctx
    torch.cuda.set_device(0)
    work = [("one_pod_balance", "balance", 1, 1024, 10000), ("one_pod_random", "random", 1, 1024, 10000),
            ("pods_balance", "balance", 256, 256, 1000), ("pods_random", "random", 256, 256, 1000)]
    ctx = bppo.Context(cfg, device=0)
    try:
        for wname, net, n_pods, E, games in work:
            if a.only and a.only != wname:
                continue

            def run():
                return evaluate_episodes_ctx(ctx, [nets[net]] * n_pods, None, games, E, sched,
                                             [1 + k for k in range(n_pods)], None, a.steps_per_launch)

            first = run()                                    # warm-up
            ts, same = [], True
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                out = run()
                ts.append(time.perf_counter() - t0)
                same = same and all(x[1:] == y[1:] and x[0].tobytes() == y[0].tobytes() for x, y in zip(out, first))
            med = statistics.median(ts)
            iters = max(o[2] for o in first)
            eps = sum(len(o[0]) for o in first)
            env_steps = sum(int(o[0]["length"].sum()) for o in first)
            print(json.dumps({"workload": wname, "net": "%s %dx%d relu" % (net, H, NL), "pods": n_pods, "envs_per_pod": E, "episodes_per_pod": games,
                              "steps_per_launch": a.steps_per_launch, "ms": _fmt(ts), "loop_iterations": iters,
                              "us_per_iteration": round(1e6 * med / iters, 2),
                              "mean_length": round(env_steps / eps, 1), "episodes_per_sec": round(eps / med, 1),
                              "env_steps_per_sec": round(env_steps / med, 1), "identical_games": same}), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
