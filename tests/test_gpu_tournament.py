"""The grouped actor forward of the evaluation loop, and whole tournaments on the device.

Grouped forward (bppo_debug_forward_groups): mode 1, one launch per layer over all models'
row groups, equals mode 0, one model after the other, bit for bit -- a row's result depends
on no other row, and the per-element arithmetic is k_gemm<GEMM_FWD>'s -- and mode 0 equals the
public bppo_forward with that model's parameters set.

Tournaments: bppo.run_tournament with its default device engine equals the same tournament
with the CPU restatement (tests/eval_ref.py) as engine in every pod, bye, game and statistic;
tests/tournament_cases.py holds the shared case and its CPU result, computed once."""
import numpy as np
import pytest

f32 = np.float32

# the group sizes of the mixed case: empty groups first, in the middle and last, and group
# boundaries inside what would be one 128-row tile
SIZES = [0, 1, 127, 128, 129, 0, 33, 300, 0]
NETS = {
    # Connect Four MLP 86 -> 512 -> 512 -> 7 relu: the 128 x 128 shape, K > KC = 256
    "c4_512": dict(preset="connect_four", hidden_size=512, num_hidden=2),
    # 64-wide tanh MLP: the BN = 64 shape and the tanh pass (the 7-wide head: BN = 32)
    "c4_tanh64": dict(preset="connect_four", hidden_size=64, num_hidden=2, activation="tanh"),
    # Liar's Dice CTDE actor 270 -> 256 -> 256 -> 49: input at + G = 120 of rows of ld 390
    "ld_ctde256": dict(preset="liars_dice_ctde", hidden_size=256, num_hidden=2, critic_hidden_size=64,
                       critic_num_hidden=2, reward_shaping_coef=0.0),
}


def _cfg(net, rows):
    import bppo
    kw = dict(NETS[net])
    return bppo.make_config(kw.pop("preset"), num_envs=max(rows, 8), num_steps=4, num_minibatches=1, num_epochs=1, **kw)


def _norm(D, seed, count):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=D) * 0.1, (rng.random(D) + 0.5) * count, float(count))


def _case(net, sizes, special):
    """-> (cfg, models, normalizers, gbase, xc).  special: model 2 gets an obs normalizer, model 3
    one with count 1 (not applied), model 6 is the random player"""
    import bppo
    rows = int(sum(sizes))
    cfg = _cfg(net, rows)
    K = len(sizes)
    # x 3: logits of order 1, so last bits matter
    base = [(bppo.orthogonal_init(cfg, seed=70 + k) * f32(3.0)).astype(f32) for k in range(min(K, 9))]
    rng = np.random.default_rng(5)
    models = [base[k] if k < len(base) else (base[k % len(base)] * f32(1.0 + 0.01 * k)).astype(f32) for k in range(K)]
    norms = [None] * K
    ctx_dims = {"connect_four": (86, 0), "liars_dice": (270, 120)}[cfg["env"]]
    D, G = ctx_dims
    if special:
        norms[2] = _norm(D, 902, 500.0)
        norms[3] = _norm(D, 903, 1.0)
        models[6] = None
    gbase = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    xc = rng.normal(size=(rows, G + D)).astype(f32)
    return cfg, models, norms, gbase, xc


def _both_modes(net, sizes, special):
    import bppo
    from bppo.eval import debug_forward_groups
    cfg, models, norms, gbase, xc = _case(net, sizes, special)
    ctx = bppo.Context(cfg, device=0)
    try:
        a = debug_forward_groups(ctx, 0, models, norms, gbase, xc)
        b = debug_forward_groups(ctx, 1, models, norms, gbase, xc)
    finally:
        ctx.close()
    return models, gbase, a, b


@pytest.mark.gpu
@pytest.mark.parametrize("net", list(NETS))
def test_grouped_forward_equals_the_per_model_loop(net):
    models, gbase, a, b = _both_modes(net, SIZES, True)
    assert a.shape == (sum(SIZES), b.shape[1]) and np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the random player's rows are zero, every row of every other group was written
    assert not a[gbase[6]:gbase[7]].any()
    for k in (1, 2, 3, 4, 7):
        assert a[gbase[k]:gbase[k + 1]].any(axis=1).all(), k


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [[1] * 64, [700]], ids=["64x1", "1x700"])
def test_grouped_forward_many_models_and_one_model(sizes):
    models, gbase, a, b = _both_modes("c4_512", sizes, False)
    assert np.isfinite(a).all() and a.any(axis=1).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("net", ["c4_512", "ld_ctde256"])
def test_per_model_loop_equals_bppo_forward(net):
    """mode 0 is the public forward: groups 4 (129 rows) and 7 (300 rows), which have no normalizer"""
    import bppo
    from bppo.eval import debug_forward_groups
    cfg, models, norms, gbase, xc = _case(net, SIZES, True)
    ctx = bppo.Context(cfg, device=0)
    try:
        a = debug_forward_groups(ctx, 0, models, norms, gbase, xc)
        G = ctx.priv_dim
        ac = bppo.ActorCritic(ctx)
        for k in (4, 7):
            rows = xc[gbase[k]:gbase[k + 1]]
            ac.set_params(models[k])
            lg, _ = ac.forward(rows[:, G:], rows[:, :G] if G else None)
            assert np.array_equal(lg.view(np.uint32), a[gbase[k]:gbase[k + 1]].view(np.uint32)), k
    finally:
        ctx.close()


@pytest.mark.gpu
def test_grouped_forward_applies_each_models_normalizer():
    """the same parameters on the same rows: with a normalizer, with one of count 1, without"""
    import bppo
    from bppo.eval import debug_forward_groups
    cfg = _cfg("c4_tanh64", 120)
    p = (bppo.orthogonal_init(cfg, seed=3) * f32(3.0)).astype(f32)
    x = np.random.default_rng(8).normal(size=(40, 86)).astype(f32)
    xc = np.concatenate([x, x, x])
    norms = [_norm(86, 1, 500.0), _norm(86, 1, 1.0), None]
    gbase = np.array([0, 40, 80, 120], np.int32)
    ctx = bppo.Context(cfg, device=0)
    try:
        a = debug_forward_groups(ctx, 0, [p, p, p], norms, gbase, xc)
        b = debug_forward_groups(ctx, 1, [p, p, p], norms, gbase, xc)
    finally:
        ctx.close()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(b[40:80], b[80:120]) and not np.array_equal(b[0:40], b[80:120])


# ------------------------------------------------------------------- tournaments ---
@pytest.mark.gpu
def test_device_tournament_equals_the_cpu_restatement():
    """the SMALL case (tests/tournament_cases.py; tests/test_tournament.py checks that its pods
    end by num_games inside max_steps): default engine against the restatement as engine"""
    from tournament_cases import run_small, small_cpu
    want, _ = small_cpu()
    got, _ = run_small(None, device=0)
    assert got.use_swiss and got.num_rounds == want.num_rounds == 3
    assert got.byes == want.byes and got.pod_seeds == want.pod_seeds
    assert len(got.pods) == len(want.pods) == 9
    for (r1, p1, g1), (r2, p2, g2) in zip(got.pods, want.pods):
        assert (r1, p1) == (r2, p2)
        assert g1 == g2, (r1, p1)                                   # placements game by game
    for a, b in zip(got.contestants, want.contestants):
        assert a is not b and a.name == b.name
        assert a.swiss_points == b.swiss_points and a.placement_counts == b.placement_counts
        assert a.draw_count == b.draw_count and a.games_played == b.games_played
        assert a.opponents_faced == b.opponents_faced and a.has_bye == b.has_bye
    assert got.standings() == want.standings()
    ra, rb = got.ratings, want.ratings
    assert [(r.rating, r.uncertainty) for r in ra.ratings] == [(r.rating, r.uncertainty) for r in rb.ratings]
    assert ra.stats.converged == rb.stats.converged and ra.stats.iterations_used == rb.stats.iterations_used
    assert got.results("t")["rankings"] == want.results("t")["rankings"]


@pytest.mark.gpu
def test_round_of_70_contestants_is_cut_into_two_calls():
    """more distinct models than one bppo_evaluate_pods call takes: 70 16-wide nets, one Swiss
    round of 35 pods, 2 envs and 2 games per pod, against the same pods and seeds on the restatement"""
    import bppo
    from test_gpu_eval import MAX_STEPS
    from tournament_cases import SCHED, CpuEngine, c4_models
    cfg, desc, params = c4_models(range(200, 270), hidden=16)

    def contestants():
        return [bppo.Contestant(f"step_{i:08d}", model=i, initial_seed=float(i)) for i in range(70)]

    sched = bppo.TempSchedule(*SCHED)
    eng = bppo.DeviceEngine(cfg, list(range(70)), params, None, 2, 2, sched, 0, MAX_STEPS)
    try:
        got = bppo.run_tournament(cfg, contestants(), params, None, 2, 2, sched, seed=9, rounds=1, engine=eng,
                                  rating_backend="host")
    finally:
        eng.close()
    assert got.use_swiss and len(got.pods) == 35 and got.byes == [[]]
    assert eng.calls == [(32, 64), (3, 6)]                          # greedy in pod order: 32 pods seat 64 models
    cpu = CpuEngine(desc, list(range(70)), params, 2, 2)
    want = cpu([p for _, p, _ in got.pods], got.pod_seeds)
    assert all(r["ended_by"] == "num_games" and r["steps"] * 4 < MAX_STEPS for r in cpu.runs)
    assert [g for _, _, g in got.pods] == want
    assert len({tuple(map(tuple, g)) for g in want}) > 1


@pytest.mark.gpu
def test_cut_rounds_play_the_same_games():
    """12 contestants (11 nets and the random player), Swiss, 2 rounds: at most 4 models per
    device call against the uncut rounds"""
    import bppo
    from test_gpu_eval import MAX_STEPS
    from tournament_cases import SCHED, c4_models
    cfg, desc, params = c4_models(range(300, 311), hidden=16)

    def run(**kw):
        cs = [bppo.Contestant(f"step_{i:08d}", model=i, initial_seed=float(i)) for i in range(11)]
        cs.append(bppo.Contestant("Random", model=None, initial_seed=-1.0))
        return bppo.run_tournament(cfg, cs, params, None, 6, 4, bppo.TempSchedule(*SCHED), seed=77, rounds=2,
                                   format="swiss", rating_backend="host", max_steps=MAX_STEPS, **kw)

    whole, cut = run(), run(max_models_per_call=4)
    assert len(whole.pods) == 12 and all(len(g) == 6 for _, _, g in whole.pods)
    assert whole.pods == cut.pods and whole.byes == cut.byes and whole.pod_seeds == cut.pod_seeds
    assert [c.swiss_points for c in whole.contestants] == [c.swiss_points for c in cut.contestants]
    assert [r.rating for r in whole.ratings.ratings] == [r.rating for r in cut.ratings.ratings]
