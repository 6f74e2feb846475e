"""Every create / destroy path gives back the device and pinned memory it took.  The library
counts the allocations and bytes its owners (bppo::DeviceMem) hold, in
this process (bppo_debug_device_memory); each case reads the counters, does its work on tiny
objects, and finds both back at the first reading.  The card's free memory is not used: on
a shared card it moves under other jobs."""
import ctypes as C
import gc

import numpy as np
import pytest

import bppo
import bppo._lib as L

pytestmark = pytest.mark.gpu

N, T = 64, 8
SMALL = dict(num_envs=N, num_steps=T, num_epochs=2, num_minibatches=2)


def live():
    """(live allocations, live bytes)"""
    a, b = C.c_int64(-1), C.c_int64(-1)
    assert L.lib().bppo_debug_device_memory(C.byref(a), C.byref(b)) == L.OK
    return a.value, b.value


@pytest.fixture
def baseline():
    gc.collect()        # a context an earlier test left to the collector goes now, not mid-test
    base = live()
    yield base
    gc.collect()
    assert live() == base


def _one_update(cfg, prepare=None):
    tr = bppo.Trainer(cfg)
    try:
        if prepare:
            prepare(tr.ctx)
        held = live()
        tr.train_update()
        assert live() == held        # an update allocates nothing that stays
    finally:
        tr.close()
    return held


def test_fused_cartpole_64x2_relu_three_times(baseline):
    """the Gumbel buffer, the reset pool, d_rowA / d_rowB"""
    cfg = bppo.make_config("cartpole", hidden_size=64, num_hidden=2, activation="relu", **SMALL)
    held = []
    for _ in range(3):
        held.append(_one_update(cfg))
        assert live() == baseline
    assert held[0][0] > baseline[0] and held[0][1] > baseline[1]
    assert held[1] == held[0] and held[2] == held[0]


def test_fused_cartpole_16x1_tanh_popart_obs_norm_ev_reference(baseline):
    """PopArt's buffers, the obs normalizer, the pinned buffers of explained-variance mode 1"""
    cfg = bppo.make_config("cartpole", hidden_size=16, num_hidden=1, activation="tanh", normalize_values=True,
                           normalize_obs=True, **SMALL)
    plain = _one_update(cfg)
    with_ev = _one_update(cfg, lambda ctx: ctx.set_explained_variance_mode(1))
    assert with_ev[0] == plain[0] + 3 and with_ev[1] == plain[1] + 3 * 4 * T * N
    assert live() == baseline


def test_cartpole_on_the_wide_path(baseline):
    """hidden 48 is not a fused width: the GEMM path and its scratch"""
    _one_update(bppo.make_config("cartpole", hidden_size=48, num_hidden=2, **SMALL))
    assert live() == baseline


def test_connect_four_cnn_smallest(baseline):
    _one_update(bppo.make_config("connect_four", network_type="cnn", num_conv_layers=1, conv_channels=[4],
                                 kernel_size=3, cnn_fc_hidden_size=16, cnn_num_fc_layers=1, **SMALL))
    assert live() == baseline


def _seats(n_opp, P, K, seed):
    rng = np.random.default_rng(seed)
    lp = rng.integers(0, P, n_opp).astype(np.int32)
    po = np.full((n_opp, P), -1, np.int32)
    for e in range(n_opp):
        for p in range(P):
            if p != lp[e]:
                po[e, p] = rng.integers(0, K)
    return lp, po, rng.integers(0, K, P - 1).astype(np.int32)


def test_liars_dice_ctde_opponents_set_twice(baseline):
    """the second bppo_opponents_set re-sizes the model set's parameters and normalizers and the
    seat buffers (1 -> 3 models, 32 -> 48 opponent envs): it releases what it replaces (the
    set's table keeps its size)"""
    cfg = bppo.make_config("liars_dice_ctde", hidden_size=64, num_hidden=2, critic_hidden_size=64, critic_num_hidden=2,
                           normalize_obs=True, **SMALL)
    tr = bppo.Trainer(cfg)
    try:
        created = live()
        counts = []
        for K, n_opp in ((1, 32), (3, 48)):
            params = np.stack([bppo.orthogonal_init(cfg, seed=100 + k) for k in range(K)])
            tr.ctx.set_opponents(params, [None] * K, n_opp, *_seats(n_opp, 4, K, seed=7 + K))
            counts.append(live())
            bppo.collect_rollouts(tr.ctx)
            assert live() == counts[-1]
        assert counts[0][0] > created[0]
        assert counts[1][0] == counts[0][0]
        np_, D = tr.ctx.n_params, tr.ctx.obs_dim
        grown = 2 * (4 * np_ + 8 * (2 * D + 1)) + (48 - 32) * (4 + 4 * 4)     # the four buffers' bytes
        assert counts[1][1] - counts[0][1] == grown
    finally:
        tr.close()
    assert live() == baseline


def test_set_allreduce_twice_on_a_popart_context(baseline):
    """PopArt's W > 1 gather scratch is sized by the world: one buffer, whatever the world"""
    cfg = bppo.make_config("cartpole", normalize_values=True, **SMALL)
    ctx = bppo.Context(cfg)
    try:
        created = live()
        ctx.set_allreduce(lambda p, n: None, 2)
        w2 = live()
        ctx.set_allreduce(lambda p, n: None, 4)
        w4 = live()
        assert w2 == (created[0] + 1, created[1] + 4 * 9 * 2)
        assert w4 == (created[0] + 1, created[1] + 4 * 9 * 4)
    finally:
        ctx.close()
    assert live() == baseline


def test_a_create_that_fails_after_allocating(baseline):
    """CTDE on Connect Four passes the configuration check, allocates the common buffers and
    is refused by the multi-player set-up; destroying the returned context frees them"""
    from bppo.host import to_struct
    s = to_struct(bppo.make_config("connect_four", network_type="ctde", hidden_size=64, **SMALL))
    h = C.c_void_p()
    st = L.lib().bppo_create(C.byref(s), 0, None, C.byref(h))
    try:
        assert st == L.ERR_ARG, (st, L.lib().bppo_last_error(h))
        assert b"CTDE needs privileged obs" in L.lib().bppo_last_error(h)
        assert live()[0] > baseline[0]         # it did allocate before it failed
    finally:
        L.lib().bppo_destroy(h)
    assert live() == baseline


def test_ratings_table_grows_and_frees(baseline):
    """600 + 600 + 1000 two-player games cross the 1024 and 2048 capacity steps; the ratings
    are those of one table fed all 2200 at once, bit for bit"""
    from bppo.ratings import RatingTable
    from test_gpu_ratings import _bits
    rng = np.random.default_rng(3)
    n = 10
    players = np.array([rng.choice(n, 2, replace=False) for _ in range(2200)], np.int32)
    places = np.tile(np.array([1, 2], np.int32), (2200, 1))
    with RatingTable() as t:
        empty = live()
        for lo, hi in ((0, 600), (600, 1200), (1200, 2200)):
            t.add_games(players[lo:hi], places[lo:hi])
        # the game arrays (3), the comparison arrays (2) and the append scratch (2), each once
        assert live()[0] == empty[0] + 7
        assert t.num_games == 2200
        batched = _bits(t.fit(n, 0))
    assert live() == baseline
    with RatingTable() as t:
        t.add_games(players, places)
        assert _bits(t.fit(n, 0)) == batched
    assert live() == baseline


def test_evaluate_pods_and_evaluate_episodes_keep_nothing(baseline):
    """the per-call buffers do not outlive the call (the smallest cases of test_gpu_eval_pods.py
    and test_gpu_eval_cartpole.py)"""
    import eval_ref_cartpole as X
    import test_gpu_eval_pods as EP
    from bppo.eval import evaluate_episodes_ctx, evaluate_pods_ctx
    env, net, n_pods, E, P, games, sched, seeds, normed, pods, pod_seeds = EP.CASES["c4_uneven"]
    cfg, params, norms = EP._models("c4_uneven")
    sched = bppo.TempSchedule(*sched)
    stats = bppo.evaluate_pods(cfg, params, norms, pods, games, E, sched, pod_seeds, max_steps=EP.MAX_STEPS)
    assert [s.total_games for s in stats] == [games] * n_pods
    assert live() == baseline
    ctx = bppo.Context(cfg)
    try:
        held = live()
        evaluate_pods_ctx(ctx, params, norms, pods, games, E, sched, pod_seeds, EP.MAX_STEPS)
        assert live() == held
    finally:
        ctx.close()
    assert live() == baseline

    case = X.CASES["freeze"]
    H, NL, act, E, games = case[0], case[1], case[2], case[6], case[7]
    model, norm = X.case_model(case)
    sched = bppo.TempSchedule(*case[8])
    stats = bppo.evaluate_episodes(X.net_config(H, NL, act), [model], [norm], games, E, sched, [case[9]],
                                   max_steps=X.MAX_STEPS)
    assert stats[0].total_games == games
    assert live() == baseline
    ctx = bppo.Context(X.net_config(H, NL, act))
    try:
        held = live()
        evaluate_episodes_ctx(ctx, [model], [norm], games, E, sched, [case[9]], X.MAX_STEPS)
        assert live() == held
    finally:
        ctx.close()
    assert live() == baseline
