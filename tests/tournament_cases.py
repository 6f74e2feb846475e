"""Shared cases of the tournament tests (tests/test_tournament.py on the CPU,
tests/test_gpu_tournament.py on the device).  TEST INFRASTRUCTURE ONLY.

SMALL: 6 Connect Four MLPs + the random player, Swiss, 3 rounds, 8 envs and 12 games per pod,
played with the CPU restatement of run_stats_mode_env (tests/eval_ref.py) as run_tournament's
engine.  Computed once and shared."""
import numpy as np

import eval_ref as R
from test_gpu_eval import MAX_STEPS, _config, _desc
from test_gpu_eval_pods import local_pod

f32 = np.float32
SCHED = (0.4, 0.0, 10, False)


def c4_models(seeds, hidden=64):
    """-> (config, oracle net description, parameters x 3 per seed)"""
    import bppo
    cfg = _config("connect_four", 8, "mlp")
    desc = _desc("connect_four", "mlp")
    if hidden != 64:
        cfg = bppo.make_config("connect_four", hidden_size=hidden, num_hidden=2, num_envs=8, num_steps=4,
                               num_minibatches=1, num_epochs=1)
        desc = R.O.mlp_desc(86, 7, hidden, 2)
    # x 3: logits of order 1, so the sampled actions depend on the logits' last bits
    return cfg, desc, [(bppo.orthogonal_init(cfg, seed=s) * f32(3.0)).astype(f32) for s in seeds]


class CpuEngine:
    """run_tournament's engine on the restatement: pod by pod, run_pod's de-duplication"""

    def __init__(self, desc, contestant_model, params, num_games, envs_per_pod, sched=SCHED):
        self.desc, self.contestant_model, self.params = desc, contestant_model, params
        self.num_games, self.envs_per_pod, self.sched = num_games, envs_per_pod, sched
        self.runs = []               # every pod's run_stats_mode output, in play order

    def __call__(self, pods, pod_seeds):
        out = []
        for pod, seed in zip(pods, pod_seeds):
            loc, seat_map = local_pod([self.contestant_model[c] for c in pod])
            models = [R.Model.random() if m is None else R.Model(self.desc, self.params[m], None) for m in loc]
            run = R.run_stats_mode("connect_four", self.envs_per_pod, len(pod), models, seat_map, self.num_games,
                                   R.TempSchedule(*self.sched), seed, max_steps=MAX_STEPS)
            self.runs.append(run)
            out.append([list(g[1][:len(pod)]) for g in run["games"]])
        return out


SMALL = dict(seeds=[11, 12, 13, 14, 15, 16], rounds=3, envs=8, games=12, seed=2024)


def small_contestants():
    import bppo
    n = len(SMALL["seeds"])
    cs = [bppo.Contestant(f"step_{100 * (i + 1):08d}", model=i, initial_seed=float(i)) for i in range(n)]
    return cs + [bppo.Contestant("Random", model=None, initial_seed=-1.0)]


def run_small(engine=None, **kw):
    """the SMALL tournament; engine None = the device"""
    import bppo
    cfg, desc, params = c4_models(SMALL["seeds"])
    cs = small_contestants()
    cpu = None
    if engine == "cpu":
        engine = cpu = CpuEngine(desc, [c.model for c in cs], params, SMALL["games"], SMALL["envs"])
    res = bppo.run_tournament(cfg, cs, params, None, SMALL["games"], SMALL["envs"], bppo.TempSchedule(*SCHED),
                              seed=SMALL["seed"], rounds=SMALL["rounds"], format="swiss", max_steps=MAX_STEPS,
                              engine=engine, rating_backend="host", **kw)
    return res, cpu


_small_cpu = []


def small_cpu():
    if not _small_cpu:
        _small_cpu.append(run_small("cpu", device=None))
    return _small_cpu[0]
