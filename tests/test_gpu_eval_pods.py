"""bppo_evaluate_pods: many evaluation matchups (pods) in one device loop.  What is pinned:
pod k equals, bit for bit, the single matchup -- the Python restatement of run_stats_mode_env
(tests/eval_ref.py) and the device's own bppo_evaluate -- run alone on E envs with the pod's
seed, the pod's local models (first-appearance order of its seats, run_pod's de-duplication,
tournament.rs:1811-1838) and the local seat map.  Everything is compared for exact equality:
integers, and f32 rewards by bit pattern.

Each pod's reference is computed once on the CPU and shared; the un-marked tests check on
the CPU alone that every pod of every case ends by reaching num_games with every game well
inside max_steps, so the device comparison cannot pass on an empty or truncated run."""
import ctypes as C
import itertools

import numpy as np
import pytest

import eval_ref as R
from test_gpu_eval import ENV_DIMS, MAX_STEPS, _config, _desc, _norm, _placement_counts

f32 = np.float32

# name: env, net, pods, envs per pod, seated players, games per pod, schedule, models (None = random;
# ints = init seeds), which models get an obs normalizer, the seats of each pod, the pods' seeds
CASES = {
    # descending global order in pod 1, one model on both seats in pod 2; the cap and the freeze
    # rule fire at different steps in different pods
    "c4_pods": ("connect_four", "mlp", 3, 16, 2, 37, (0.4, 0.0, 10, False), [11, 12, 13, None], [1],
                [[0, 1], [3, 1], [2, 2]], [201, 7777, 31337]),
    # pod 0 (two greedy nets: every env plays the same short game) is finished and frozen many
    # steps before pod 1 (random players)
    "c4_uneven": ("connect_four", "mlp", 2, 16, 2, 5, (0.0, 0.0, None, False), [11, 12, None], [],
                  [[0, 1], [2, 2]], [301, 302]),
    # more models than bppo_evaluate's 15, more pods than envs per pod
    "c4_many": ("connect_four", "mlp", 40, 2, 2, 3, (0.4, 0.0, 10, False), [50 + i for i in range(19)] + [None], [4],
                [[(7 * k) % 20, (3 * k + 1) % 20] for k in range(40)], [1000 + 17 * k for k in range(40)]),
    # a thread owns more than one env (the single-pod analogue is test_gpu_eval's c4_wide)
    "c4_big_pod": ("connect_four", "mlp", 2, 550, 2, 600, (1.0, 0.0, None, False), [11, 12], [],
                   [[0, 1], [1, 0]], [401, 402]),
    "ld_ctde_pods": ("liars_dice", "ctde", 2, 35, 4, 100, (1.0, 0.2, 6, True), [21, 22, None], [0],
                     [[0, 1, 0, 2], [2, 2, 1, 0]], [501, 502]),
    "skull3_pods": ("skull", "mlp", 2, 12, 3, 40, (1.0, 0.0, None, False), [31, 32], [1],
                    [[0, 1, 0], [1, 1, 0]], [601, 602]),
    "c4_cnn_pods": ("connect_four", "cnn", 2, 16, 2, 20, (0.4, 0.0, 10, False), [41, 42], [],
                    [[0, 1], [1, 1]], [701, 702]),
}


def _models(name, num_envs=None):
    import bppo
    env, net, n_pods, E, P, games, sched, seeds, normed, pods, pod_seeds = CASES[name]
    cfg = _config(env, n_pods * E if num_envs is None else num_envs, net, P)
    # x 3: logits of order 1, so the sampled actions depend on the logits' last bits
    params = [None if s is None else (bppo.orthogonal_init(cfg, seed=s) * f32(3.0)).astype(f32) for s in seeds]
    norms = [_norm(ENV_DIMS[env][0], 900 + k) if k in normed else None for k in range(len(seeds))]
    return cfg, params, norms


def local_pod(seats):
    """run_pod's de-duplication: -> (global models in local-slot order, local seat map)"""
    order = []
    for m in seats:
        if m not in order:
            order.append(m)
    return order, [order.index(m) for m in seats]


_refs = {}


def reference(name, k, order=None):
    """pod k of the case alone on the CPU; order: the pod's global models in another order
    than local-slot order"""
    key = (name, k, None if order is None else tuple(order))
    if key not in _refs:
        env, net, n_pods, E, P, games, sched, seeds, normed, pods, pod_seeds = CASES[name]
        cfg, params, norms = _models(name)
        d = _desc(env, net)
        loc, seat_map = local_pod(pods[k])
        if order is not None:
            loc, seat_map = list(order), [list(order).index(m) for m in pods[k]]
        models = [R.Model.random() if params[m] is None else R.Model(d, params[m], norms[m]) for m in loc]
        _refs[key] = R.run_stats_mode(env, E, P, models, seat_map, games, R.TempSchedule(*sched), pod_seeds[k],
                                      max_steps=MAX_STEPS)
    return _refs[key]


def test_local_pod():
    assert local_pod([3, 1, 3]) == ([3, 1], [0, 1, 0])
    assert local_pod([2, 2, 1, 0]) == ([2, 1, 0], [0, 0, 1, 2])


@pytest.mark.parametrize("name", list(CASES))
def test_reference_pods_end_by_num_games(name):
    n_pods, games = CASES[name][2], CASES[name][5]
    outs = [reference(name, k) for k in range(n_pods)]
    for out in outs:
        assert out["ended_by"] == "num_games" and len(out["games"]) == games
        assert out["steps"] * 4 < MAX_STEPS and out["max_len"] * 4 < MAX_STEPS
    if name == "c4_pods":
        # the draw-order rule: pod 1 seats [3, 1]; its models in ascending global order play other games
        asc = reference(name, 1, order=[1, 3])
        assert [g[1:] for g in asc["games"]] != [g[1:] for g in outs[1]["games"]]
        assert len({o["steps"] for o in outs}) > 1          # the cap fires at different steps
    if name == "c4_uneven":
        a, b = sorted(o["steps"] for o in outs)
        assert b >= 2 * a


def _device_pods(name, max_steps=MAX_STEPS):
    import bppo
    from bppo.eval import evaluate_pods_ctx
    env, net, n_pods, E, P, games, sched, seeds, normed, pods, pod_seeds = CASES[name]
    cfg, params, norms = _models(name)
    ctx = bppo.Context(cfg, device=0)
    try:
        return evaluate_pods_ctx(ctx, params, norms, pods, games, E, bppo.TempSchedule(*sched), pod_seeds, max_steps)
    finally:
        ctx.close()


def _records_equal(a, b):
    """two device record arrays: integers equal, f32 rewards equal by bit pattern"""
    if len(a) != len(b):
        return False
    if not np.array_equal(a["total_reward"].view(np.uint32), b["total_reward"].view(np.uint32)):
        return False
    return all(np.array_equal(a[f], b[f]) for f in ("placement", "length", "env_index", "perm_index", "step"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_every_pod_matches_its_reference(name):
    n_pods, P, games = CASES[name][2], CASES[name][4], CASES[name][5]
    out = _device_pods(name)
    assert len(out) == n_pods
    for k, (rec, pos) in enumerate(out):
        ref = reference(name, k)
        assert len(rec) == len(ref["games"]) == games, k
        assert pos == ref["rng_pos"], k
        assert R.games_equal(ref["games"], rec), k
        assert np.array_equal(_placement_counts(rec, P), ref["placements"]), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c4_pods", "skull3_pods"])
def test_every_pod_matches_the_single_matchup_path(name):
    """the device against the device's own bppo_evaluate on a context of envs_per_pod envs;
    with one pod the two calls agree outright"""
    import bppo
    from bppo.eval import evaluate_ctx, evaluate_pods_ctx
    env, net, n_pods, E, P, games, sched, seeds, normed, pods, pod_seeds = CASES[name]
    out = _device_pods(name)
    cfg, params, norms = _models(name, num_envs=E)
    ts = bppo.TempSchedule(*sched)
    ctx = bppo.Context(cfg, device=0)
    try:
        for k in range(n_pods):
            loc, seat_map = local_pod(pods[k])
            rec, pos = evaluate_ctx(ctx, [params[m] for m in loc], [norms[m] for m in loc], seat_map, games, ts,
                                    pod_seeds[k], MAX_STEPS)
            assert len(rec) == games
            assert pos == out[k][1], k
            assert _records_equal(rec, out[k][0]), k
            (rec1, pos1), = evaluate_pods_ctx(ctx, params, norms, [pods[k]], games, E, ts, [pod_seeds[k]], MAX_STEPS)
            assert pos1 == pos and _records_equal(rec1, rec), k
    finally:
        ctx.close()


def _raw_call(ctx, K, params, is_random, n_pods, E, seeds, seats, n_games, num_games=5, max_steps=MAX_STEPS):
    import bppo._lib as L
    cfg = L.EvalConfig(num_games=num_games, max_steps=max_steps, seed=0, temp_initial=1.0, temp_final=0.0,
                       temp_cutoff=-1, temp_decay=0)
    games = (L.EvalGame * (max(num_games, 1) * max(n_pods, 1)))()
    p = lambda a: None if a is None else a.ctypes.data       # noqa: E731
    return L.lib().bppo_evaluate_pods(ctx.h, C.byref(cfg), K, p(params), None, None, None, p(is_random), n_pods, E,
                                      p(seeds), p(seats), C.cast(games, C.c_void_p), max(num_games, 1), p(n_games),
                                      None)


@pytest.mark.gpu
def test_argument_checks():
    import bppo
    import bppo._lib as L
    from bppo.eval import evaluate_pods_ctx
    sched = bppo.TempSchedule(1.0)
    cp = bppo.Context(bppo.make_config("cartpole", num_envs=8, num_steps=4, num_minibatches=1), device=0)
    try:
        with pytest.raises(bppo.BppoError) as e:
            L.check(_raw_call(cp, 1, np.zeros((1, cp.n_params), f32), None, 2, 4, np.zeros(2, np.uint64),
                              np.zeros((2, 1), np.int32), np.zeros(2, np.int32)), cp.h)
        assert e.value.status == L.ERR_UNSUPPORTED and "CartPole" in str(e.value)
    finally:
        cp.close()
    name = "c4_pods"
    env, net, n_pods, E, P, games, _, _, _, pods, pod_seeds = CASES[name]
    cfg, params, norms = _models(name)
    K = len(params)
    pa = np.stack([np.zeros_like(params[0]) if p is None else p for p in params])
    rnd = np.array([p is None for p in params], np.int32)
    seeds = np.array(pod_seeds, np.uint64)
    seats = np.array(pods, np.int32)
    ng = np.zeros(n_pods, np.int32)
    ctx = bppo.Context(cfg, device=0)
    try:
        bad_hi, bad_lo = seats.copy(), seats.copy()
        bad_hi[1, 0], bad_lo[2, 1] = K, -1
        for args, msg in (((K, pa, rnd, n_pods, E, None, seats, ng), "NULL"),
                          ((K, pa, rnd, n_pods, E, seeds, None, ng), "NULL"),
                          ((K, pa, rnd, n_pods, E, seeds, seats, None), "NULL"),
                          ((K, pa, rnd, n_pods, E + 1, seeds, seats, ng), "num_envs"),
                          ((K, pa, rnd, n_pods - 1, E, seeds, seats, ng), "num_envs"),
                          ((K, pa, rnd, n_pods, E, seeds, bad_hi, ng), "out of range"),
                          ((K, pa, rnd, n_pods, E, seeds, bad_lo, ng), "out of range"),
                          ((0, pa, rnd, n_pods, E, seeds, seats, ng), "1..64 models"),
                          ((65, pa, rnd, n_pods, E, seeds, seats, ng), "1..64 models"),
                          ((K, None, rnd, n_pods, E, seeds, seats, ng), "parameters required")):
            with pytest.raises(bppo.BppoError) as e:
                L.check(_raw_call(ctx, *args), ctx.h)
            assert e.value.status == L.ERR_ARG and msg in str(e.value), msg
        with pytest.raises(bppo.BppoError) as e:       # no Connect Four game ends within 3 moves
            evaluate_pods_ctx(ctx, params, norms, pods, 5, E, sched, pod_seeds, 3)
        assert e.value.status == L.ERR_ARG and "max_steps" in str(e.value)
        # the context still works
        out = evaluate_pods_ctx(ctx, params, norms, pods, games, E, bppo.TempSchedule(*CASES[name][6]), pod_seeds,
                                MAX_STEPS)
        for k, (rec, pos) in enumerate(out):
            ref = reference(name, k)
            assert pos == ref["rng_pos"] and R.games_equal(ref["games"], rec), k
    finally:
        ctx.close()


def _ref_stats(ref, P):
    from bppo.eval import EvalStats
    st = EvalStats(P)
    for cr, pl, length, env, pi, step in ref["games"]:
        st.record_with_rewards(pl[:P], cr[:P], length)
    return st


@pytest.mark.gpu
def test_python_surface():
    """bppo.evaluate_pods -> one EvalStats per pod; bppo.run_round -> the pods' placements"""
    import bppo
    name = "c4_pods"
    env, net, n_pods, E, P, games, sched, seeds, normed, pods, pod_seeds = CASES[name]
    cfg, params, norms = _models(name)
    cfg = dict(cfg, num_envs=1)                 # evaluate_pods sizes the context itself
    ts = bppo.TempSchedule(*sched)
    stats = bppo.evaluate_pods(cfg, params, norms, pods, games, E, ts, seeds=pod_seeds)
    rnd = bppo.run_round(cfg, params, norms, pods, games, E, ts, seeds=pod_seeds)
    assert len(stats) == len(rnd) == n_pods
    for k, st in enumerate(stats):
        ref = reference(name, k)
        want = _ref_stats(ref, P)
        assert st.total_games == games and st.rng_word_pos == ref["rng_pos"]
        assert np.array_equal(st.placements, ref["placements"]) and np.array_equal(st.placements, want.placements)
        assert [st.wins(c) for c in range(P)] == [want.wins(c) for c in range(P)]
        assert [st.losses(c) for c in range(P)] == [want.losses(c) for c in range(P)]
        assert st.draws() == want.draws()
        assert st.games == [(g[3], g[4], g[5]) for g in ref["games"]]
        assert rnd[k]["contestants"] == list(pods[k])
        assert rnd[k]["games"] == [list(g[1][:P]) for g in ref["games"]]


def test_evaluate_pods_signature():
    import inspect

    import bppo
    sig = inspect.signature(bppo.evaluate_pods)
    assert list(sig.parameters) == ["config", "models", "normalizers", "pods", "num_games", "envs_per_pod",
                                    "temp_schedule", "seeds", "seed", "device", "max_steps"]


def test_round_robin_and_swiss_points():
    import bppo
    assert bppo.round_robin_pods(5, 3) == [list(p) for p in itertools.combinations(range(5), 3)]
    assert len(bppo.round_robin_pods(8, 2)) == 28
    assert bppo.swiss_points([1, 2, 3, 4]) == [3.0, 2.0, 1.0, 0.0]
    assert bppo.swiss_points([1, 1, 3, 4]) == [2.5, 2.5, 1.0, 0.0]
    assert bppo.swiss_points([1, 2, 2, 4]) == [3.0, 1.5, 1.5, 0.0]
    assert bppo.swiss_points([1, 1, 1, 1]) == [1.5] * 4
    assert bppo.swiss_points([]) == []
