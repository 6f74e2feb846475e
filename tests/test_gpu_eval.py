"""bppo_evaluate on the device against the Python restatement of run_stats_mode_env
(tests/eval_ref.py, eval.rs:1621-1877).  Everything is compared for exact equality --
integers, and f32 rewards by bit pattern: given bit-exact logits (wide_forward_actor,
test_gpu_wide.py::test_opponent_pool_rollout_update_bit_exact) every quantity is discrete.
Compared: the game list, the final RNG word position, the placement counts.

Each case's reference is computed once on the CPU and shared; the un-marked tests check
on the CPU alone that every case ends by reaching num_games (not by running out of
active envs) with every game well inside max_steps."""
import ctypes as C

import numpy as np
import pytest

import eval_ref as R
from test_eval_ref import ROW_SHAPES, SAMPLER_POS, SAMPLER_SEED, hook_sample, reference_rows

f32 = np.float32
MAX_STEPS = 2000
ENV_DIMS = {"connect_four": (86, 7), "liars_dice": (270, 49), "skull": (135, 33)}


def _config(env, N, net, player_count=4):
    import bppo
    kw = dict(num_envs=N, num_steps=4, num_minibatches=1, num_epochs=1)
    if env == "connect_four" and net == "cnn":
        return bppo.make_config("connect_four", network_type="cnn", num_conv_layers=2, conv_channels=[8, 8],
                                kernel_size=3, cnn_fc_hidden_size=32, cnn_num_fc_layers=1, **kw)
    if env == "connect_four":
        return bppo.make_config("connect_four", hidden_size=64, num_hidden=2, **kw)
    if env == "liars_dice":
        return bppo.make_config("liars_dice_ctde", hidden_size=64, num_hidden=2, critic_hidden_size=64,
                                critic_num_hidden=2, reward_shaping_coef=0.0, **kw)
    return bppo.make_config("skull", hidden_size=64, num_hidden=2, player_count=player_count, **kw)


def _desc(env, net):
    D, A = ENV_DIMS[env]
    if net == "cnn":
        return R.O.cnn_desc(7, [8, 8], 3, 32, 1)
    if env == "liars_dice":
        return R.O.ctde_desc(270, 120, 49, 64, 2, 64, 2)
    return R.O.mlp_desc(D, A, 64, 2)


def _norm(D, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=D) * 0.1, (rng.random(D) + 0.5) * 500.0, 500.0)


# name: env, net, N, seated players, num_games, schedule, models (None = random; ints = init seeds),
# which models get an obs normalizer, seat_model, seed
CASES = {
    "c4_mixed": ("connect_four", "mlp", 16, 2, 37, (0.4, 0.0, 10, False), [11, 12], [1], [0, 1], 101),
    "c4_freeze": ("connect_four", "mlp", 16, 2, 5, (0.0, 0.0, None, False), [11, 12], [], [0, 1], 102),
    "c4_wide": ("connect_four", "mlp", 1100, 2, 1200, (1.0, 0.0, None, False), [11, 12], [], [0, 1], 103),
    "ld_ctde": ("liars_dice", "ctde", 70, 4, 100, (1.0, 0.0, None, False), [21, 22, None], [0], [0, 1, 0, 2], 104),
    "ld_decay": ("liars_dice", "ctde", 70, 4, 100, (1.0, 0.2, 6, True), [21, 22, None], [0], [0, 1, 0, 2], 105),
    "skull_3": ("skull", "mlp", 24, 3, 40, (1.0, 0.0, None, False), [31, 32], [1], [0, 1, 0], 106),
    "skull_6": ("skull", "mlp", 8, 6, 10, (1.0, 0.0, None, False), [31, 32, None], [], [0, 1, 2, 0, 1, 0], 107),
    "c4_cnn": ("connect_four", "cnn", 16, 2, 20, (0.4, 0.0, 10, False), [41, 42], [], [0, 1], 108),
    # seats that name the models out of ascending order, and a model that is not seated: the draws
    # still go over the models in ascending index, not in the seats' first-appearance order
    "c4_desc": ("connect_four", "mlp", 16, 2, 37, (0.4, 0.0, 10, False), [11, 12, 13], [], [2, 0], 109),
    "ld_desc": ("liars_dice", "ctde", 35, 4, 60, (1.0, 0.2, 6, True), [21, None, 22], [2], [2, 0, 2, 1], 110),
}
# case: (steps, longest game, final word position) of the reference run
DESC_RUNS = {"c4_desc": (50, 23, 368), "ld_desc": (65, 37, 1640)}


def _models(name):
    import bppo
    env, net, N, P, games, sched, seeds, normed, seat_model, seed = CASES[name]
    cfg = _config(env, N, net, P)
    # x 3: logits of order 1 rather than the policy head's 0.01-gain initial ones, so the
    # sampled actions depend on the logits' last bits
    params = [None if s is None else (bppo.orthogonal_init(cfg, seed=s) * f32(3.0)).astype(f32) for s in seeds]
    norms = [_norm(ENV_DIMS[env][0], 900 + k) if k in normed else None for k in range(len(seeds))]
    return cfg, params, norms


_refs = {}


def reference(name, order=None):
    """order: the seated models listed in another order than ascending index (the seats renumbered to match)"""
    key = (name, None if order is None else tuple(order))
    if key not in _refs:
        env, net, N, P, games, sched, seeds, normed, seat_model, seed = CASES[name]
        cfg, params, norms = _models(name)
        d = _desc(env, net)
        models = [R.Model.random() if p is None else R.Model(d, p, norms[k]) for k, p in enumerate(params)]
        if order is not None:
            models, seat_model = [models[m] for m in order], [list(order).index(m) for m in seat_model]
        _refs[key] = R.run_stats_mode(env, N, P, models, seat_model, games, R.TempSchedule(*sched), seed,
                                      max_steps=MAX_STEPS)
    return _refs[key]


@pytest.mark.parametrize("name", list(CASES))
def test_reference_run_ends_by_num_games(name):
    out = reference(name)
    games = CASES[name][4]
    assert out["ended_by"] == "num_games" and len(out["games"]) == games
    assert out["steps"] * 4 < MAX_STEPS and out["max_len"] * 4 < MAX_STEPS
    if name == "c4_freeze":
        assert sorted(g[3] for g in out["games"]) == [11, 12, 13, 14, 15] and out["rng_pos"] == 2
    if name == "c4_mixed":          # the cap and the freeze rule fire in the last round
        assert len({g[5] for g in out["games"]}) > 1 and out["games"][-1][5] == out["steps"] - 1
    if name in DESC_RUNS:
        assert (out["steps"], out["max_len"], out["rng_pos"]) == DESC_RUNS[name]
        # the draw-order rule: the seated models in first-appearance order of the seats play other games
        seats = CASES[name][8]
        first = reference(name, order=sorted(set(seats), key=seats.index))
        assert [g[1:] for g in first["games"]] != [g[1:] for g in out["games"]]
        if name == "ld_desc":
            assert first["rng_pos"] == 1612


def _device_run(name, max_steps=MAX_STEPS):
    import bppo
    from bppo.eval import evaluate_ctx
    env, net, N, P, games, sched, seeds, normed, seat_model, seed = CASES[name]
    cfg, params, norms = _models(name)
    ctx = bppo.Context(cfg, device=0)
    try:
        return evaluate_ctx(ctx, params, norms, seat_model, games, bppo.TempSchedule(*sched), seed, max_steps)
    finally:
        ctx.close()


def _placement_counts(rec, ncp):
    out = np.zeros((ncp, ncp), np.int64)
    for g in rec:
        for c in range(ncp):
            if 0 < g["placement"][c] <= ncp:
                out[c][g["placement"][c] - 1] += 1
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("A,B,seed", ROW_SHAPES)
def test_device_sampler_matches_python_on_random_rows(A, B, seed):
    logits, masks, temps, act, used, _ = reference_rows(A, B, seed)
    a, u = hook_sample(A, logits, masks, temps, SAMPLER_SEED, SAMPLER_POS, device=1)
    assert np.array_equal(u, used)
    assert np.array_equal(a, act)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_evaluate_matches_reference(name):
    ref = reference(name)
    rec, pos = _device_run(name)
    ncp = CASES[name][3]
    assert len(rec) == len(ref["games"])
    assert pos == ref["rng_pos"]
    assert R.games_equal(ref["games"], rec)
    assert np.array_equal(_placement_counts(rec, ncp), ref["placements"])
    if name == "c4_freeze":
        assert sorted(rec["env_index"].tolist()) == [11, 12, 13, 14, 15] and pos == 2


@pytest.mark.gpu
def test_evaluate_python_surface():
    """bppo.evaluate -> EvalStats: placement counts, wins / losses / draws, lengths"""
    import bppo
    name = "c4_mixed"
    env, net, N, P, games, sched, seeds, normed, seat_model, seed = CASES[name]
    cfg, params, norms = _models(name)
    ref = reference(name)
    st = bppo.evaluate(cfg, params, norms, seat_model, games, bppo.TempSchedule(*sched), seed)
    assert st.total_games == games and st.rng_word_pos == ref["rng_pos"]
    assert np.array_equal(st.placements, ref["placements"])
    assert st.episode_lengths == [g[2] for g in ref["games"]]
    assert st.wins(0) + st.wins(1) + st.draws() == games
    assert st.wins(0) == st.losses(1) and st.wins(1) == st.losses(0)
    assert st.games == [(g[3], g[4], g[5]) for g in ref["games"]]


@pytest.mark.gpu
def test_argument_checks():
    import bppo
    import bppo._lib as L
    from bppo.eval import evaluate_ctx
    sched = bppo.TempSchedule(1.0)
    cp = bppo.Context(bppo.make_config("cartpole", num_envs=8, num_steps=4, num_minibatches=1), device=0)
    try:
        with pytest.raises(bppo.BppoError) as e:
            evaluate_ctx(cp, [np.zeros(cp.n_params, f32)], None, [0], 2, sched, 1, 10)
        assert e.value.status == L.ERR_UNSUPPORTED and "CartPole" in str(e.value)
    finally:
        cp.close()
    cfg, params, norms = _models("c4_freeze")
    ctx = bppo.Context(cfg, device=0)
    try:
        for seats, msg in (([0, 1, 0], "n_checkpoints"), ([0], "n_checkpoints"), ([0, 2], "out of range"),
                           ([-1, 0], "out of range")):
            with pytest.raises(bppo.BppoError) as e:
                evaluate_ctx(ctx, params, norms, seats, 5, sched, 1, 100)
            assert e.value.status == L.ERR_ARG and msg in str(e.value)
        with pytest.raises(bppo.BppoError) as e:       # no Connect Four game ends within 3 moves
            evaluate_ctx(ctx, params, norms, [0, 1], 5, sched, 1, 3)
        assert e.value.status == L.ERR_ARG and "max_steps" in str(e.value)
        rec, pos = evaluate_ctx(ctx, params, norms, [0, 1], 5, sched, 1, MAX_STEPS)   # the context still works
        assert len(rec) == 5
    finally:
        ctx.close()


@pytest.mark.gpu
def test_training_is_untouched_by_an_evaluation():
    """two identical contexts train one update; one of them then plays an evaluation; both
    reset their VecEnv and train on: parameters, metrics and the main RNG position agree
    bit for bit (the evaluation leaves parameters, optimizer, normalizers and RNG alone)"""
    import bppo
    from bppo.eval import evaluate_ctx
    cfg = bppo.make_config("connect_four", hidden_size=64, num_hidden=2, num_envs=16, num_steps=8, num_minibatches=2,
                           num_epochs=2)
    p0 = bppo.orthogonal_init(cfg, seed=5)
    trs = [bppo.Trainer(cfg, device=0, params=p0) for _ in range(2)]
    try:
        for tr in trs:
            bppo.train_step(tr.ctx, 1e-3, 0.01)
        other = (bppo.orthogonal_init(cfg, seed=6) * f32(3.0)).astype(f32)
        rec, _ = evaluate_ctx(trs[0].ctx, [other, None], None, [0, 1], 9, bppo.TempSchedule(1.0), 3, MAX_STEPS)
        assert len(rec) == 9
        out = []
        for tr in trs:
            bppo.VecEnv.new(tr.ctx)                     # bppo_vecenv_reset
            _, m = bppo.train_step(tr.ctx, 1e-3, 0.01)
            out.append((tr.model.get_params(), m, tr.ctx.rng_pos()))
        assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
        assert out[0][2] == out[1][2]
        for k, v in out[0][1].items():
            assert np.array_equal(np.asarray(v, f32).view(np.uint32), np.asarray(out[1][1][k], f32).view(np.uint32)), k
    finally:
        for tr in trs:
            tr.close()
