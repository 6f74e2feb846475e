"""Tournament rounds on the device, timed.  Reported, not gated.

    python scripts/bench_tournament.py [--workload rr|swiss|both] [--repeats 5]
    python scripts/bench_tournament.py --against-tree DIR [--alternations 2]

Connect Four, the configs/connect_four.toml MLP (2 x 512), the env's default temperature
schedule, 64 envs and 256 games per pod:
    rr      the 28 round-robin pods of 8 checkpoints (scripts/eval_pods_timing.py's round)
    swiss   round 1 of a Swiss tournament of 64 checkpoints seeded 0..63: 32 pods, all 64
            models move in every loop iteration
Each workload is timed two ways, each after one warm-up, `repeats` invocations:
    call    bppo.evaluate_pods: context creation, the models' upload, the loop, the results
    loop    bppo.eval.evaluate_pods_ctx on one context made before: upload, loop and results
Printed are the median (min - max) seconds per round and ms per loop step of both, and a
digest of the games played.

--against-tree DIR compares with another commit: DIR is a built checkout of it (its own
burn-ppo_amd/bppo package and libbppo.so, e.g. `git worktree add DIR <commit>` and
`make -C DIR/burn-ppo_amd`).  This script then runs in fresh child processes alternately on
DIR's package and on this tree's (it uses only what both have: make_config, orthogonal_init,
TempSchedule, Context, evaluate_pods, evaluate_pods_ctx), pools each side's invocations,
checks that both played the same games and prints both sides and the two conditions of
section 7h."""
import argparse
import hashlib
import itertools
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def workloads():
    """name -> (models, pods).  swiss: swiss_pods' round 1 of 64 contestants with initial_seed
    = index (tournament.rs:779-791): ranked 63..0, pod i = [ranked[i], ranked[i + 32]]"""
    rr = [list(p) for p in itertools.combinations(range(8), 2)]
    swiss = [[63 - i, 31 - i] for i in range(32)]
    return {"rr": (8, rr), "swiss": (64, swiss)}


def _digest(stats_or_recs):
    h = hashlib.sha256()
    for x in stats_or_recs:
        h.update(repr(x).encode())
    return h.hexdigest()


def run_workload(name, repeats, tree=ROOT, envs=64, games=256, seed=1):
    """tree: the checkout whose bppo package (and library) is timed"""
    sys.path.insert(0, os.path.join(tree, "burn-ppo_amd"))
    import numpy as np
    import torch
    import bppo
    from bppo.eval import evaluate_pods_ctx
    torch.cuda.set_device(0)
    n_models, pods = workloads()[name]
    if name == "swiss" and hasattr(bppo, "swiss_pods"):
        cs = [bppo.Contestant(f"step_{i:08d}", model=i, initial_seed=float(i)) for i in range(64)]
        assert bppo.swiss_pods(cs, 2) == pods
    cfg = bppo.make_config("connect_four", num_envs=envs, num_steps=8, num_minibatches=1, num_epochs=1)
    params = [(bppo.orthogonal_init(cfg, seed=s + 1) * np.float32(3.0)).astype(np.float32) for s in range(n_models)]
    sched = bppo.TempSchedule.env_default("connect_four")
    seeds = [seed + k for k in range(len(pods))]

    def call():
        stats = bppo.evaluate_pods(cfg, params, None, pods, games, envs, sched, seeds=seeds)
        return [(st.games, st.game_outcomes, st.rng_word_pos) for st in stats]

    ctx = bppo.Context(dict(cfg, num_envs=len(pods) * envs), device=0)

    def loop():
        out = evaluate_pods_ctx(ctx, params, None, pods, games, envs, sched, seeds)
        return [([(int(g["env_index"]), int(g["perm_index"]), int(g["step"])) for g in rec],
                 [[int(x) for x in g["placement"][:2]] for g in rec], pos) for rec, pos in out]

    res = {"workload": name, "models": n_models, "pods": len(pods), "envs_per_pod": envs, "games_per_pod": games}
    digests = {}
    try:
        for key, fn in (("call", call), ("loop", loop)):
            fn()                                                # warm-up
            ts = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                played = fn()
                ts.append(time.perf_counter() - t0)
                digests.setdefault(key, set()).add(_digest(played))
                res["loop_steps"] = max(g[2] for p in played for g in p[0]) + 1
            res[key + "_seconds"] = ts
    finally:
        ctx.close()
    if any(len(d) != 1 for d in digests.values()):
        raise SystemExit("two invocations played different games")
    res["games_digest"] = [digests[key].pop() for key in ("call", "loop")]
    return res


def summary(ts, steps):
    med = statistics.median(ts)
    return {"median_s": round(med, 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4),
            "median_ms_per_step": round(1e3 * med / steps, 4), "min_ms_per_step": round(1e3 * min(ts) / steps, 4),
            "max_ms_per_step": round(1e3 * max(ts) / steps, 4), "invocations": len(ts)}


def child(tree, workload, repeats):
    env = dict(os.environ)
    env.pop("BPPO_LIB_PATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", workload, "--repeats", str(repeats),
                          "--raw", "--tree", tree], env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--workload", choices=["rr", "swiss", "both"], default="both")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--against-tree", default=None, help="a built checkout of another commit to alternate with")
    p.add_argument("--alternations", type=int, default=2)
    p.add_argument("--raw", action="store_true", help="print the invocations' seconds (child mode)")
    p.add_argument("--tree", default=ROOT, help="the checkout whose bppo package is timed (child mode)")
    a = p.parse_args()
    names = ["rr", "swiss"] if a.workload == "both" else [a.workload]
    if a.raw:
        print(json.dumps(run_workload(names[0], a.repeats, os.path.abspath(a.tree))), flush=True)
        return
    for name in names:
        if not a.against_tree:
            r = run_workload(name, a.repeats)
            for key in ("call", "loop"):
                r[key] = summary(r.pop(key + "_seconds"), r["loop_steps"])
            print(json.dumps(r), flush=True)
            continue
        sides = {"against": [], "this": []}
        for _ in range(a.alternations):
            sides["against"].append(child(os.path.abspath(a.against_tree), name, a.repeats))
            sides["this"].append(child(ROOT, name, a.repeats))
        runs = sides["against"] + sides["this"]
        out = {k: v for k, v in runs[0].items() if not k.endswith("_seconds") and k != "games_digest"}
        out["same_games"] = len({tuple(r["games_digest"]) for r in runs}) == 1 and len({r["loop_steps"] for r in runs}) == 1
        for side, rs in sides.items():
            out[side] = {key: summary([t for r in rs for t in r[key + "_seconds"]], rs[0]["loop_steps"])
                         for key in ("call", "loop")}
        for key in ("call", "loop"):
            if name == "rr":
                out[f"condition_1_{key}_median_s_not_above_parent_max"] = \
                    out["this"][key]["median_s"] <= out["against"][key]["max_s"]
            else:
                out[f"condition_2_{key}_median_ms_per_step_below_parent_min"] = \
                    out["this"][key]["median_ms_per_step"] < out["against"][key]["min_ms_per_step"]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
