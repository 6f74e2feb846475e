"""bppo_evaluate_episodes (csrc/eval_cartpole.hip): single-player stats mode for CartPole on the
device against the Python restatement of run_stats_mode_env (tests/eval_ref.py with the CartPole
env of tests/eval_ref_cartpole.py).  Every comparison is exact: the records through
eval_ref.games_equal (integers equal, f32 totals by bit pattern), the final RNG word position,
the game count.  Given bit-exact logits every quantity is discrete.

Each reference is computed once on the CPU and shared; test_eval_cartpole_ref.py pins, on the
CPU alone, that every case ends by num_games and exercises what it is here for."""
import ctypes as C

import numpy as np
import pytest

import eval_ref as R
import eval_ref_cartpole as X

f32 = np.float32
pytestmark = pytest.mark.gpu


def _device(cases, steps_per_launch=0, max_steps=X.MAX_STEPS):
    """cases of one net shape as the pods of one call -> [(records, word position, loop steps)]"""
    import bppo
    from bppo.eval import evaluate_episodes_ctx
    H, NL, act = cases[0][:3]
    assert all(c[:3] == (H, NL, act) and c[6:9] == cases[0][6:9] for c in cases)
    E, games, sched = cases[0][6:9]
    models = [X.case_model(c) for c in cases]
    ctx = bppo.Context(X.net_config(H, NL, act), device=0)
    try:
        return evaluate_episodes_ctx(ctx, [m for m, _ in models], [n for _, n in models], games, E,
                                     bppo.TempSchedule(*sched), [c[9] for c in cases], max_steps, steps_per_launch)
    finally:
        ctx.close()


def _records_equal(a, b):
    if len(a) != len(b):
        return False
    if not np.array_equal(a["total_reward"].view(np.uint32), b["total_reward"].view(np.uint32)):
        return False
    return all(np.array_equal(a[f], b[f]) for f in ("placement", "length", "env_index", "perm_index", "step"))


def _matches(ref, out):
    rec, pos, steps = out
    return (len(rec) == len(ref["games"]) and pos == ref["rng_pos"] and steps == ref["steps"]
            and R.games_equal(ref["games"], rec))


@pytest.mark.parametrize("name", list(X.CASES))
def test_case_matches_reference(name):
    ref = X.reference(name)
    out, = _device([X.CASES[name]])
    rec, pos, steps = out
    assert len(rec) == len(ref["games"]) == X.CASES[name][7]
    assert pos == ref["rng_pos"]
    assert steps == ref["steps"]
    assert R.games_equal(ref["games"], rec)
    if name in ("greedy", "greedy_zero", "truncation"):
        assert pos == 2
    if name == "truncation":
        assert rec["length"].tolist() == [500] * 10 and rec["total_reward"][:, 0].tolist() == [500.0] * 10


@pytest.mark.parametrize("shape", X.POD_SHAPES, ids=lambda s: "%dx%d%s" % s)
def test_pods_match_reference_and_the_single_pod_call(shape):
    cases = [X.pod_case(shape, k) for k in range(X.N_PODS)]
    outs = _device(cases)
    assert len(outs) == X.N_PODS
    for k, out in enumerate(outs):
        assert _matches(X.pod_reference(shape, k), out), k
        alone, = _device([cases[k]])
        assert alone[1:] == out[1:] and _records_equal(alone[0], out[0]), k


def test_steps_per_launch_does_not_change_the_games():
    ref = X.reference("default")
    outs = [_device([X.CASES["default"]], steps_per_launch=s)[0] for s in (1, 7, 0)]
    for out in outs:
        assert _matches(ref, out)
        assert out[1:] == outs[0][1:] and _records_equal(out[0], outs[0][0])


def _raw(ctx, n_pods, E, params, seeds, n_games, num_games=5, max_steps=X.MAX_STEPS, pos=None, steps=None):
    import bppo._lib as L
    cfg = L.EvalConfig(num_games=num_games, max_steps=max_steps, seed=0, temp_initial=0.3, temp_final=0.0,
                       temp_cutoff=-1, temp_decay=0)
    games = (L.EvalGame * (max(num_games, 1) * max(n_pods, 1)))()
    p = lambda a: None if a is None else a.ctypes.data       # noqa: E731
    return L.lib().bppo_evaluate_episodes(ctx.h, C.byref(cfg), n_pods, E, p(params), None, None, None, p(seeds), 0,
                                          C.cast(games, C.c_void_p), max(num_games, 1), p(n_games), p(pos), p(steps))


def test_argument_checks():
    import bppo
    import bppo._lib as L
    from bppo.eval import evaluate_episodes_ctx
    ng, seeds = np.zeros(2, np.int32), np.array([1, 2], np.uint64)

    def refused(ctx, status, msg, *args, **kw):
        with pytest.raises(bppo.BppoError) as e:
            L.check(_raw(ctx, *args, **kw), ctx.h)
        assert e.value.status == status and msg in str(e.value), (msg, str(e.value))

    for over in (dict(hidden_size=48), dict(num_hidden=3), dict(split_networks=True)):     # GEMM-path CartPole nets
        wide = bppo.Context(bppo.make_config("cartpole", num_envs=8, num_steps=4, num_minibatches=1, **over), device=0)
        try:
            refused(wide, L.ERR_UNSUPPORTED, "fused CartPole nets", 2, 4, np.zeros((2, wide.n_params), f32), seeds, ng)
        finally:
            wide.close()
    c4 = bppo.Context(bppo.make_config("connect_four", hidden_size=64, num_hidden=2, num_envs=8, num_steps=4,
                                       num_minibatches=1), device=0)
    try:
        refused(c4, L.ERR_UNSUPPORTED, "bppo_evaluate", 2, 4, np.zeros((2, c4.n_params), f32), seeds, ng)
    finally:
        c4.close()
    case = X.CASES["default"]
    ctx = bppo.Context(X.net_config(*case[:3]), device=0)
    try:
        pa = np.stack([X.case_model(case)[0]] * 2)
        refused(ctx, L.ERR_ARG, "n_pods", 0, 4, pa, seeds, ng)
        refused(ctx, L.ERR_ARG, "n_pods", 1025, 4, pa, seeds, ng)
        refused(ctx, L.ERR_ARG, "envs_per_pod", 2, 0, pa, seeds, ng)
        refused(ctx, L.ERR_ARG, "envs_per_pod", 2, 16385, pa, seeds, ng)
        refused(ctx, L.ERR_ARG, "NULL", 2, 4, pa, None, ng)
        refused(ctx, L.ERR_ARG, "NULL", 2, 4, None, seeds, ng)
        refused(ctx, L.ERR_ARG, "NULL", 2, 4, pa, seeds, None)
        # max_steps too small: the error, and where the run stood
        ref = X.reference("default")
        cut = 20
        pos, steps = np.zeros(2, np.uint64), np.zeros(2, np.int32)
        refused(ctx, L.ERR_ARG, "max_steps", 1, case[6], pa[:1], np.array([case[9]], np.uint64), ng,
                num_games=case[7], max_steps=cut, pos=pos, steps=steps)
        want = [g for g in ref["games"] if g[5] < cut]
        assert 0 < len(want) < case[7]
        assert ng[0] == len(want) and steps[0] == cut
        assert pos[0] == 2 + sum(d for d, _ in ref["draws_per_step"][:cut])
        # num_games = 0: no iteration, position 2
        assert _raw(ctx, 2, 4, pa, seeds, ng, num_games=0, pos=pos, steps=steps) == L.OK
        assert ng.tolist() == [0, 0] and pos.tolist() == [2, 2] and steps.tolist() == [0, 0]
        # the context still works
        out, = evaluate_episodes_ctx(ctx, [pa[0]], None, case[7], case[6], bppo.TempSchedule(*case[8]), [case[9]],
                                     X.MAX_STEPS)
        assert _matches(ref, out)
    finally:
        ctx.close()


def test_training_is_undisturbed_by_an_evaluation():
    """two contexts with one seed: one runs train_step, an evaluation, train_step, the other
    train_step, train_step.  The observation right after the evaluation, the second step's rollout
    buffers, the parameters and the RNG position agree bit for bit."""
    import bppo
    from bppo.eval import evaluate_episodes_ctx
    cfg = bppo.make_config("cartpole", hidden_size=64, num_hidden=2, num_envs=96, num_steps=16, num_minibatches=2,
                           num_epochs=2, normalize_obs=True)
    p0 = bppo.orthogonal_init(cfg, seed=5)
    trs = [bppo.Trainer(cfg, device=0, params=p0) for _ in range(2)]
    try:
        for tr in trs:
            bppo.train_step(tr.ctx, 1e-3, 0.01)
        case = X.CASES["default"]
        out, = evaluate_episodes_ctx(trs[0].ctx, [X.case_model(case)[0]], None, case[7], case[6],
                                     bppo.TempSchedule(*case[8]), [case[9]], X.MAX_STEPS)
        assert _matches(X.reference("default"), out)
        obs = [bppo.VecEnv(tr.ctx).get_observations() for tr in trs]
        assert np.array_equal(obs[0].view(np.uint32), obs[1].view(np.uint32))
        res = []
        for tr in trs:
            _, m = bppo.train_step(tr.ctx, 1e-3, 0.01)
            buf = bppo.RolloutBuffer(tr.ctx)
            res.append(dict(params=tr.model.get_params(), rng=tr.ctx.rng_pos(), actions=buf.actions,
                            **{k: getattr(buf, k) for k in ("observations", "rewards", "dones", "values", "log_probs",
                                                            "advantages", "returns")}))
        assert res[0]["rng"] == res[1]["rng"]
        for k in res[0]:
            if k != "rng":
                a, b = np.ascontiguousarray(res[0][k]), np.ascontiguousarray(res[1][k])
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
    finally:
        for tr in trs:
            tr.close()


def _ref_stats(ref):
    import bppo
    st = bppo.EvalStats(1)
    for cr, pl, length, env, pi, step in ref["games"]:
        st.record_with_rewards(pl[:1], cr[:1], length)
    return st


def test_python_surface(tmp_path):
    """bppo.evaluate_episodes, bppo.evaluate (CartPole) and bppo.evaluate_checkpoints give the
    same stats as the restatement; best is the pod with the larger restated mean"""
    import bppo
    from bppo import checkpoint as ck
    shape = X.POD_SHAPES[0]
    H, NL, act = shape
    pods = [0, 2]                                            # pod 2 carries an obs normalizer
    cases = [X.pod_case(shape, k) for k in pods]
    refs = [X.pod_reference(shape, k) for k in pods]
    want = [_ref_stats(r) for r in refs]
    models = [X.case_model(c) for c in cases]
    cfg = X.net_config(H, NL, act)
    ts = bppo.TempSchedule(*cases[0][8])
    seeds = [c[9] for c in cases]
    stats = bppo.evaluate_episodes(cfg, [m for m, _ in models], [n for _, n in models], X.POD_GAMES, X.POD_ENVS, ts,
                                   seeds=seeds)
    one = bppo.evaluate(dict(cfg, num_envs=X.POD_ENVS), [models[1][0]], [models[1][1]], [0], X.POD_GAMES, ts, seeds[1])
    dirs = []
    for k, (params, norm) in enumerate(models):
        d = tmp_path / ("step_%08d" % k)
        d.mkdir()
        ck.save_model(cfg, params, str(d / "model.mpk"))
        (d / "metadata.json").write_text(ck.CheckpointMetadata.for_config(cfg, k, 0.0).to_json())
        if norm is not None:
            (d / "normalizer.json").write_text(ck.to_json_pretty(
                {"mean": [float(v) for v in norm[0]], "var": [float(v) for v in norm[1]], "count": float(norm[2]),
                 "clip": ck.F32(10.0)}))
        dirs.append(str(d))
    from_dirs, best = bppo.evaluate_checkpoints(dirs, X.POD_GAMES, X.POD_ENVS, ts, seeds=seeds)
    for got in (stats, from_dirs, [None, one]):
        for k, st in enumerate(got):
            if st is None:
                continue
            assert st.total_games == X.POD_GAMES and st.rng_word_pos == refs[k]["rng_pos"]
            assert st.game_rewards == want[k].game_rewards and st.episode_lengths == want[k].episode_lengths
            assert st.games == [(g[3], g[4], g[5]) for g in refs[k]["games"]]
            assert st.reward_summary() == want[k].reward_summary()
            assert np.array_equal(st.placements, [[X.POD_GAMES]])
    means = [w.reward_summary()["mean"] for w in want]
    assert means[0] != means[1] and best == int(np.argmax(means))
