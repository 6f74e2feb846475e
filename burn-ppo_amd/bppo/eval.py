"""Stats-mode evaluation (eval.rs): play N games between checkpoints on the device.

    TempSchedule            eval.rs:76-216  (get_temp, env defaults, argument errors)
    generate_permutations   eval.rs:1591-1612 (Heap's algorithm, as written)
    rewards_to_placements   eval.rs:276-306
    evaluate                eval.rs:1621-1877 run_stats_mode_env -> EvalStats (eval.rs:315-390)
    evaluate_pods           many such matchups in one device loop, one RNG seed per pod
    evaluate_episodes       single-player stats mode (CartPole): pods of one checkpoint each in one
                            kernel launch sequence -> EvalStats.reward_summary (eval.rs:416-469)
    evaluate_checkpoints    checkpoint directories as the pods of one evaluate_episodes call

The games run inside libbppo (bppo_evaluate, csrc/eval.hip; bppo_evaluate_episodes,
csrc/eval_cartpole.hip) on a context of their own.  Checkpoint loading stays with
bppo.checkpoint; ratings and printing are not part of this module."""
import ctypes as C

import numpy as np

from . import _lib as L
from .ppo import Context, _pack_models

# E::EVAL_TEMP and E::EVAL_TEMP_CUTOFF (connect_four.rs:219-221, liars_dice.rs:454,
# skull.rs:1052; the trait's defaults are 0.3 and None, env.rs:53-58)
EVAL_TEMP = {"connect_four": 0.4, "liars_dice": 1.0, "skull": 1.0}
EVAL_TEMP_CUTOFF = {"connect_four": (10, 0.0), "liars_dice": None, "skull": None}


_libm = None


def _fmaf(a, b, c):
    """f32 fused multiply-add (Rust's f32::mul_add) from the platform libm: one rounding"""
    global _libm
    if _libm is None:
        import ctypes.util
        _libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.fmaf.restype = C.c_float
        _libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]
    return _libm.fmaf(float(a), float(b), float(c))


class TempSchedule:
    """eval.rs:76-91: initial, final_temp, cutoff (None = constant), decay."""

    def __init__(self, initial, final_temp=0.0, cutoff=None, decay=False):
        self.initial = np.float32(initial)
        self.final_temp = np.float32(final_temp)
        self.cutoff = None if cutoff is None else int(cutoff)
        self.decay = bool(decay)

    @classmethod
    def from_args(cls, env, temp=None, temp_final=None, temp_cutoff=None, no_temp_cutoff=False,
                  temp_decay=False):
        """from_args_with_env_defaults (eval.rs:99-141): the env's EVAL_TEMP / EVAL_TEMP_CUTOFF
        unless overridden; temp_final or temp_decay without any cutoff is an error."""
        default = EVAL_TEMP.get(env, 0.3)
        env_cutoff = EVAL_TEMP_CUTOFF.get(env)
        if no_temp_cutoff:
            return cls(default if temp is None else temp, 0.0, None, False)
        cutoff = temp_cutoff if temp_cutoff is not None else (env_cutoff[0] if env_cutoff else None)
        if cutoff is None:
            if temp_final is not None:
                raise ValueError("--temp-final requires --temp-cutoff to be set (or env default)")
            if temp_decay:
                raise ValueError("--temp-decay requires --temp-cutoff to be set (or env default)")
        final = temp_final if temp_final is not None else (env_cutoff[1] if env_cutoff else 0.0)
        return cls(default if temp is None else temp, final, cutoff, temp_decay)

    @classmethod
    def env_default(cls, env):
        return cls.from_args(env)

    def get_temp(self, move_num):
        """eval.rs:200-216 in f32: the decay is one fused multiply-add."""
        if self.cutoff is None:
            return self.initial
        if move_num >= self.cutoff:
            return self.final_temp
        if not self.decay:
            return self.initial
        t = np.float32(move_num) / np.float32(self.cutoff)
        return np.float32(_fmaf(t, self.final_temp - self.initial, self.initial))


def generate_permutations(n):
    """eval.rs:1591-1612: all permutations of 0..n by Heap's algorithm, in its order."""
    out, arr = [], list(range(n))

    def heap_permute(k):
        if k == 1:
            out.append(list(arr))
            return
        heap_permute(k - 1)
        for i in range(k - 1):
            j = i if k % 2 == 0 else 0
            arr[j], arr[k - 1] = arr[k - 1], arr[j]
            heap_permute(k - 1)

    heap_permute(n)
    return out


def rewards_to_placements(rewards):
    """eval.rs:276-306: 1 = first; rewards within 1e-6 of a tie group's first share its place."""
    r = [np.float32(x) for x in rewards]
    order = sorted(range(len(r)), key=lambda i: -r[i])      # stable, descending
    pl = [0] * len(r)
    cur, i = 1, 0
    while i < len(order):
        first = r[order[i]]
        tied = 0
        while i + tied < len(order) and abs(np.float32(r[order[i + tied]] - first)) < np.float32(1e-6):
            tied += 1
        for j in range(tied):
            pl[order[i + j]] = cur
        cur += tied
        i += tied
    return pl


class EvalStats:
    """eval.rs:315-390: placement counts per checkpoint, the game list, episode lengths."""

    def __init__(self, num_players):
        self.num_players = num_players
        self.placements = np.zeros((num_players, num_players), np.int64)
        self.total_games = 0
        self.game_rewards = []
        self.episode_lengths = []
        self.game_outcomes = []
        self.games = []          # (env_index, perm_index, step) of each recorded game
        self.rng_word_pos = 0

    def record_with_rewards(self, outcome, rewards, length):
        self.game_rewards.append([float(x) for x in rewards])
        self.episode_lengths.append(int(length))
        self.record(outcome)

    def record(self, outcome):
        self.total_games += 1
        self.game_outcomes.append(list(outcome))
        for i, place in enumerate(outcome):
            if 0 < place <= self.num_players:
                self.placements[i][place - 1] += 1

    def wins(self, player):
        return sum(1 for o in self.game_outcomes if o[player] == 1 and sum(p == 1 for p in o) == 1)

    def losses(self, player):
        return sum(1 for o in self.game_outcomes if o[player] == self.num_players)

    def draws(self):
        return sum(1 for o in self.game_outcomes if all(p == 1 for p in o))

    def reward_summary(self):
        """the numbers print_single_player_summary prints (eval.rs:416-469) for player 0, in f64:
        mean, population std, min, max, p25 / p50 / p75 as sorted[len * q / 100] clamped to the last
        index, and the episode lengths' mean / min / max.  None without reward data."""
        rewards = sorted(float(r[0]) for r in self.game_rewards if len(r))
        if not rewards:
            return None
        n = len(rewards)
        mean = sum(rewards) / n
        var = sum((r - mean) ** 2 for r in rewards) / n
        out = dict(mean=mean, std=var ** 0.5, min=rewards[0], max=rewards[-1])
        for q in (25, 50, 75):
            out[f"p{q}"] = rewards[min(n * q // 100, n - 1)]
        if self.episode_lengths:
            out.update(length_mean=sum(self.episode_lengths) / len(self.episode_lengths),
                       length_min=min(self.episode_lengths), length_max=max(self.episode_lengths))
        return out


def _eval_config(num_games, num_envs, temp_schedule, seed, max_steps):
    if max_steps is None:
        # every env plays at most ceil(num_games / num_envs) + 1 games; no game of these envs
        # runs longer than a few hundred moves
        max_steps = 1000 * (num_games // max(num_envs, 1) + 2)
    return L.EvalConfig(num_games=int(num_games), max_steps=int(max_steps), seed=int(seed),
                        temp_initial=float(temp_schedule.initial), temp_final=float(temp_schedule.final_temp),
                        temp_cutoff=-1 if temp_schedule.cutoff is None else int(temp_schedule.cutoff),
                        temp_decay=int(temp_schedule.decay))


def _stats(rec, pos, ncp):
    stats = EvalStats(ncp)
    for g in rec:
        stats.record_with_rewards([int(x) for x in g["placement"][:ncp]], g["total_reward"][:ncp], g["length"])
        stats.games.append((int(g["env_index"]), int(g["perm_index"]), int(g["step"])))
    stats.rng_word_pos = pos
    return stats


def evaluate_ctx(ctx, models, normalizers, seat_model, num_games, temp_schedule, seed, max_steps=None):
    """bppo_evaluate on an existing context (its VecEnv is reset and overwritten).
    models[k]: a flat parameter vector, or None for the random player; normalizers[k]:
    (mean, m2, count) or None.  -> (games as a numpy record array, rng word position)"""
    K = len(models)
    params, mean, m2, cnt, is_random = _pack_models(ctx, models, normalizers)
    seats = np.ascontiguousarray(seat_model, np.int32)
    cfg = _eval_config(num_games, ctx.N, temp_schedule, seed, max_steps)
    games = (L.EvalGame * max(int(num_games), 1))()
    n = C.c_int32()
    pos = C.c_uint64()
    st = L.lib().bppo_evaluate(ctx.h, C.byref(cfg), K, params.ctypes.data, mean.ctypes.data, m2.ctypes.data,
                               cnt.ctypes.data, is_random.ctypes.data, seats.ctypes.data, len(seats),
                               C.cast(games, C.c_void_p), int(num_games), C.byref(n), C.byref(pos))
    L.check(st, ctx.h)
    rec = np.frombuffer(games, dtype=np.dtype(L.EvalGame), count=max(int(num_games), 1)).copy()
    return rec[:min(n.value, int(num_games))], pos.value


def evaluate(config, models, normalizers, seat_model, num_games, temp_schedule=None, seed=0, device=0,
             max_steps=None):
    """run_stats_mode_env (eval.rs:1621-1877) with config["num_envs"] parallel games on a
    context of its own: models[seat_model[c]] plays checkpoint c (None = the random
    player), every permutation of the seats in turn.  -> EvalStats"""
    if temp_schedule is None:
        temp_schedule = TempSchedule.env_default(config["env"])
    if config["env"] == "cartpole":
        # single-player stats mode: one pod of config["num_envs"] envs on the fused kernel
        if [int(m) for m in seat_model] != [0]:
            raise ValueError("CartPole has one player: seat_model must be [0]")
        stats, = evaluate_episodes(config, [models[0]], [normalizers[0]] if normalizers else None, num_games,
                                   config["num_envs"], temp_schedule, seeds=[seed], device=device,
                                   max_steps=max_steps)
        return stats
    ctx = Context(config, device=device)
    try:
        rec, pos = evaluate_ctx(ctx, models, normalizers, seat_model, num_games, temp_schedule, seed, max_steps)
        ncp = len(seat_model)
    finally:
        ctx.close()
    return _stats(rec, pos, ncp)


def evaluate_pods_ctx(ctx, models, normalizers, pods, num_games, envs_per_pod, temp_schedule, seeds, max_steps=None):
    """bppo_evaluate_pods on an existing context of len(pods) * envs_per_pod envs (its VecEnv
    is reset and overwritten).  models / normalizers as in evaluate_ctx, shared by all pods;
    pods[k]: the global model index of each checkpoint of pod k; seeds[k]: pod k's RNG seed;
    num_games per pod.  -> [(games as a numpy record array, rng word position)] per pod,
    each equal to evaluate_ctx alone on that pod's models with that seed"""
    K, n_pods, cap = len(models), len(pods), max(int(num_games), 1)
    params, mean, m2, cnt, is_random = _pack_models(ctx, models, normalizers)
    seats = np.ascontiguousarray(pods, np.int32).reshape(n_pods, -1)
    if seats.shape[1] != ctx.seats:
        raise ValueError(f"every pod seats {ctx.seats} checkpoints, got {seats.shape[1]}")
    pod_seeds = np.ascontiguousarray([int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], np.uint64)
    if len(pod_seeds) != n_pods:
        raise ValueError("one seed per pod")
    cfg = _eval_config(num_games, envs_per_pod, temp_schedule, 0, max_steps)
    games = (L.EvalGame * (cap * n_pods))()
    n = np.zeros(n_pods, np.int32)
    pos = np.zeros(n_pods, np.uint64)
    st = L.lib().bppo_evaluate_pods(ctx.h, C.byref(cfg), K, params.ctypes.data, mean.ctypes.data, m2.ctypes.data,
                                    cnt.ctypes.data, is_random.ctypes.data, n_pods, int(envs_per_pod),
                                    pod_seeds.ctypes.data, seats.ctypes.data, C.cast(games, C.c_void_p), cap,
                                    n.ctypes.data, pos.ctypes.data)
    L.check(st, ctx.h)
    rec = np.frombuffer(games, dtype=np.dtype(L.EvalGame), count=cap * n_pods).copy().reshape(n_pods, cap)
    return [(rec[k, :min(int(n[k]), int(num_games))], int(pos[k])) for k in range(n_pods)]


def debug_forward_groups(ctx, mode, models, normalizers, gbase, xc):
    """bppo_debug_forward_groups: the evaluation loop's actor forward of models[k] (None = the
    random player, zero logits) on rows [gbase[k], gbase[k + 1]) of xc [rows][G + D].  mode 0: one
    model after the other; mode 1: the grouped launches.  -> logits [rows][A]"""
    K = len(models)
    params, mean, m2, cnt, is_random = _pack_models(ctx, models, normalizers)
    gb = np.ascontiguousarray(gbase, np.int32)
    if gb.shape != (K + 1,):
        raise ValueError("gbase has one entry per model and the end")
    rows = int(gb[-1])
    xc = np.ascontiguousarray(xc, np.float32)
    if rows < 0 or xc.size != rows * (ctx.priv_dim + ctx.obs_dim):
        raise ValueError("xc is [gbase[-1]][priv_dim + obs_dim]")
    logits = np.zeros((rows, ctx.num_actions), np.float32)
    L.check(L.lib().bppo_debug_forward_groups(ctx.h, int(mode), K, params.ctypes.data, mean.ctypes.data,
                                              m2.ctypes.data, cnt.ctypes.data, is_random.ctypes.data, gb.ctypes.data,
                                              xc.ctypes.data, logits.ctypes.data), ctx.h)
    return logits


def evaluate_pods(config, models, normalizers, pods, num_games, envs_per_pod, temp_schedule=None, seeds=None, seed=0,
                  device=0, max_steps=None):
    """Many matchups in one device loop (a tournament round): pod k plays num_games games
    between models[pods[k][c]] for c in 0..P on envs_per_pod envs of a context of its own
    with len(pods) * envs_per_pod envs.  Every pod has its own RNG, StdRng(seeds[k]) (default
    seed + k), so pod k's EvalStats equals evaluate() alone on that pod with that seed; the
    reference's one RNG handed from pod to pod is evaluate() pod after pod.  -> [EvalStats]"""
    if temp_schedule is None:
        temp_schedule = TempSchedule.env_default(config["env"])
    pods = [tuple(int(m) for m in p) for p in pods]
    if seeds is None:
        seeds = [seed + k for k in range(len(pods))]
    cfg = dict(config)
    cfg["num_envs"] = len(pods) * int(envs_per_pod)
    ctx = Context(cfg, device=device)
    try:
        out = evaluate_pods_ctx(ctx, models, normalizers, pods, num_games, envs_per_pod, temp_schedule, seeds,
                                max_steps)
    finally:
        ctx.close()
    return [_stats(rec, pos, len(pods[k])) for k, (rec, pos) in enumerate(out)]


def evaluate_episodes_ctx(ctx, models, normalizers, num_games, envs_per_pod, temp_schedule, seeds, max_steps=None,
                          steps_per_launch=0):
    """bppo_evaluate_episodes on an existing CartPole context, which is read for its net shape
    and stream only (its envs, RNG, parameters and buffers are not touched).  Pod k plays num_games
    episodes of models[k] (a flat parameter vector; normalizers[k]: (mean, m2, count) or None) on
    envs_per_pod envs with StdRng(seeds[k]).  -> [(games as a numpy record array, rng word
    position, loop iterations)] per pod"""
    n_pods, cap = len(models), max(int(num_games), 1)
    if any(m is None for m in models):
        raise ValueError("single-player evaluation has no random player: every model needs parameters")
    params, mean, m2, cnt, _ = _pack_models(ctx, models, normalizers)
    pod_seeds = np.ascontiguousarray([int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], np.uint64)
    if len(pod_seeds) != n_pods:
        raise ValueError("one seed per pod")
    if max_steps is None:
        # an episode lasts at most 500 steps and an env records at most ceil(num_games / envs) + 1
        max_steps = 500 * (int(num_games) // max(int(envs_per_pod), 1) + 2)
    cfg = _eval_config(num_games, envs_per_pod, temp_schedule, 0, max_steps)
    games = (L.EvalGame * (cap * max(n_pods, 1)))()
    n = np.zeros(max(n_pods, 1), np.int32)
    pos = np.zeros(max(n_pods, 1), np.uint64)
    steps = np.zeros(max(n_pods, 1), np.int32)
    st = L.lib().bppo_evaluate_episodes(ctx.h, C.byref(cfg), n_pods, int(envs_per_pod), params.ctypes.data,
                                        mean.ctypes.data, m2.ctypes.data, cnt.ctypes.data, pod_seeds.ctypes.data,
                                        int(steps_per_launch), C.cast(games, C.c_void_p), cap, n.ctypes.data,
                                        pos.ctypes.data, steps.ctypes.data)
    L.check(st, ctx.h)
    rec = np.frombuffer(games, dtype=np.dtype(L.EvalGame), count=cap * n_pods).copy().reshape(n_pods, cap)
    return [(rec[k, :min(int(n[k]), int(num_games))], int(pos[k]), int(steps[k])) for k in range(n_pods)]


def evaluate_episodes(config, models, normalizers, num_games, envs_per_pod, temp_schedule=None, seeds=None, seed=0,
                      device=0, max_steps=None, steps_per_launch=0):
    """Single-player stats mode (run_stats_mode_env with num_players = 1, eval.rs:1621-1877) for
    CartPole: pod k plays num_games episodes of models[k] on envs_per_pod envs with its own RNG,
    StdRng(seeds[k]) (default seed + k), all pods in one kernel launch sequence on a small
    context of its own.  The default schedule is the trait's (0.3, no cutoff).  -> [EvalStats],
    whose reward_summary() gives print_single_player_summary's numbers"""
    if temp_schedule is None:
        temp_schedule = TempSchedule.env_default(config["env"])
    if seeds is None:
        seeds = [seed + k for k in range(len(models))]
    cfg = dict(config)
    cfg.update(num_envs=8, num_steps=4, num_minibatches=1, num_epochs=1)   # the context lends its net shape only
    ctx = Context(cfg, device=device)
    try:
        out = evaluate_episodes_ctx(ctx, models, normalizers, num_games, envs_per_pod, temp_schedule, seeds,
                                    max_steps, steps_per_launch)
    finally:
        ctx.close()
    return [_stats(rec, pos, 1) for rec, pos, _ in out]


def evaluate_checkpoints(dirs, num_games, envs_per_pod, temp_schedule=None, seeds=None, seed=0, device=0,
                         max_steps=None):
    """Every checkpoint directory of a CartPole run (metadata.json, model.mpk and, when the run
    normalized observations, normalizer.json; bppo.checkpoint) as one pod of a single
    evaluate_episodes call.  The directories must describe one architecture.
    -> ([EvalStats] per directory, index of the best mean return)"""
    import json
    import os

    from . import checkpoint as ck
    from .host import make_config
    dirs = list(dirs)
    if not dirs:
        raise ValueError("no checkpoint directories")
    metas = [ck.load_metadata(d) for d in dirs]

    def arch(m):
        return (m.env_name, m.network_type, m.hidden_size, m.num_hidden, m.activation, m.split_networks)

    if any(arch(m) != arch(metas[0]) for m in metas):
        raise ValueError("evaluate_checkpoints: the checkpoints differ in architecture")
    m0 = metas[0]
    if m0.env_name != "cartpole":
        raise ValueError("evaluate_checkpoints: single-player (CartPole) checkpoints only")
    config = make_config("cartpole", hidden_size=m0.hidden_size, num_hidden=m0.num_hidden, activation=m0.activation,
                         network_type=m0.network_type, split_networks=m0.split_networks)
    models = [ck.load_model(os.path.join(d, "model.mpk")) for d in dirs]
    norms = []
    for d in dirs:
        p = os.path.join(d, "normalizer.json")
        if os.path.exists(p):
            with open(p) as f:
                j = json.load(f)
            norms.append((np.asarray(j["mean"], np.float64), np.asarray(j["var"], np.float64), float(j["count"])))
        else:
            norms.append(None)
    stats = evaluate_episodes(config, models, norms, num_games, envs_per_pod, temp_schedule, seeds, seed, device,
                              max_steps)
    means = [s.reward_summary()["mean"] if s.total_games else float("-inf") for s in stats]
    return stats, int(np.argmax(means))
