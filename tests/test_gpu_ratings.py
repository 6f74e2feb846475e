"""Plackett-Luce ratings on the device (csrc/ratings.hip, bppo.ratings) against the restatement
tests/pl_ref.py, whose results and order spreads are recorded in tests/golden/ratings_ref.json
(scripts/make_ratings_golden.py; tests/test_ratings_ref.py checks the file on the CPU).

The bar of every compared quantity is 16 x the largest spread of the restatement's own outputs
over 8 random orderings of the same games: summation order is the only freedom the device takes,
the factor is for its exp / log differing from libm's by an ulp on top."""
import json
import os

import numpy as np
import pytest

import bppo
import bppo._lib as L
import pl_ref
from bppo.ratings import RatingTable, compute_ratings

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ratings_ref.json")))
BAR = 16.0


def _split(games):
    return [g[0] for g in games], [g[1] for g in games]


def _bits(res):
    return (np.array([r.rating for r in res.ratings]).tobytes(), np.array([r.uncertainty for r in res.ratings]).tobytes(),
            res.gammas.tobytes(), res.stats.converged, res.stats.iterations_used,
            np.float64(res.stats.final_delta).tobytes())


@pytest.fixture(scope="module")
def fits():
    """one device fit per fixture, shared"""
    out = {}
    for name in pl_ref.FIXTURES:
        n, games, anchor = pl_ref.fixture(name)
        with RatingTable() as t:
            t.add_games(*_split(games))
            out[name] = t.fit(n, anchor)
    return out


@pytest.mark.parametrize("name", pl_ref.FIXTURES)
def test_device_fit_matches_the_restatement(fits, name):
    n, games, anchor = pl_ref.fixture(name)
    ref, res = GOLDEN[name], fits[name]
    st = res.stats
    assert (st.converged, st.iterations_used, st.n_games, st.n_comparisons) == \
        (ref["converged"], ref["iterations_used"], len(games), ref["n_comparisons"])
    played = pl_ref.count_games_per_player(games, n)
    rating = np.array([r.rating for r in res.ratings])
    unc = np.array([r.uncertainty for r in res.ratings])
    d_rating = np.abs(rating - np.array(ref["rating"])).max()
    d_unc = np.abs(unc - np.array(ref["uncertainty"])).max()
    d_gamma = np.abs(res.gammas - np.array(ref["gamma"])).max()
    d_delta = abs(st.final_delta - ref["final_delta"])
    sp = ref["spread"]
    print(f"\n{name}: |d rating| {d_rating:.3e} (spread {sp['rating']:.3e})  |d uncertainty| {d_unc:.3e} "
          f"(spread {sp['uncertainty']:.3e})  |d gamma| {d_gamma:.3e} (spread {sp['gamma']:.3e})  "
          f"|d final_delta| {d_delta:.3e} (spread {sp['final_delta']:.3e})  "
          f"anchor {rating[anchor]!r} / {ref['rating'][anchor]!r}")
    for i in range(n):
        if played[i] == 0:
            assert (rating[i], unc[i]) == (1000.0, 350.0), i
    assert rating[anchor] == ref["rating"][anchor] and unc[anchor] == ref["uncertainty"][anchor] == 0.0
    assert d_rating <= BAR * sp["rating"]
    assert d_unc <= BAR * sp["uncertainty"]
    assert d_delta <= BAR * sp["final_delta"]
    if not ref["converged"]:        # the never-winning fixture: gamma after exactly 100 iterations
        assert st.iterations_used == 100 and d_gamma <= BAR * sp["gamma"]


@pytest.mark.parametrize("name", ["M", "N130", "long", "edge"])
def test_bit_reproducible(fits, name):
    """two fits of one table; the same games in one call, in three calls, and after clear()"""
    n, games, anchor = pl_ref.fixture(name)
    pl, pc = _split(games)
    want = _bits(fits[name])
    with RatingTable() as t:
        t.add_games(pl, pc)
        assert _bits(t.fit(n, anchor)) == want
        assert _bits(t.fit(n, anchor)) == want
        t.clear()
        assert t.num_games == 0
        a, b = len(games) // 3, len(games) // 2 + 1
        for lo, hi in ((0, a), (a, b), (b, len(games))):
            t.add_games(pl[lo:hi], pc[lo:hi])
        assert t.num_games == len(games)
        assert _bits(t.fit(n, anchor)) == want
        # the host backend on a device table is the restatement, bit for bit
        h = t.fit(n, anchor, backend="host")
        assert [r.rating for r in h.ratings] == GOLDEN[name]["rating"]
        assert [r.uncertainty for r in h.ratings] == GOLDEN[name]["uncertainty"]


def test_weight_three_equals_three_copies():
    n, games, anchor = pl_ref.fixture("M")
    pl, pc = _split(games)
    w = np.ones(len(games))
    w[5] = 3.0
    with RatingTable() as a, RatingTable() as b:
        a.add_games(pl, pc, w)
        b.add_games(pl[:6] + [pl[5], pl[5]] + pl[6:], pc[:6] + [pc[5], pc[5]] + pc[6:])
        ra, rb = a.fit(n, anchor), b.fit(n, anchor)
    sp = GOLDEN["M"]["spread"]
    assert ra.stats.iterations_used == rb.stats.iterations_used
    assert max(abs(x.rating - y.rating) for x, y in zip(ra.ratings, rb.ratings)) <= BAR * sp["rating"]
    assert max(abs(x.uncertainty - y.uncertainty) for x, y in zip(ra.ratings, rb.ratings)) <= BAR * sp["uncertainty"]


# ------------------------------------------------------------- add_completions ---
def _pool_ctx():
    from test_gpu_opp_completions import _trainer
    tr, _ = _trainer("connect_four", 32)
    return tr


def test_add_completions_equals_host_mapping():
    """64 envs x 32 steps of Connect Four against 3 models: the table filled on the device equals
    the table filled from bppo_opponents_completions mapped on the host; slot 1 is the learner's
    own player id, so its games are skipped (main.rs:779-782)"""
    learner, slots = 1, [0, 1, 2]
    tr = _pool_ctx()
    bppo.collect_rollouts(tr.ctx)
    comps, dropped = tr.ctx.opponent_completions()
    assert dropped == 0 and len(comps) >= 48
    pl, pc = [], []
    for c in comps:
        opp = [(slots[m], c["placements"][seat]) for seat, m in enumerate(c["position_to_opponent"]) if m >= 0]
        if all(o[0] == learner for o in opp):
            continue
        pl.append([learner] + [o[0] for o in opp])
        pc.append([c["placements"][c["learner_position"]]] + [o[1] for o in opp])
    assert 0 < len(pl) < len(comps)
    with RatingTable() as a, RatingTable() as b:
        added = a.add_completions(tr.ctx, learner, slots)
        assert added == len(pl) == a.num_games
        b.add_games(pl, pc)
        ra, rb = a.fit(3, 0), b.fit(3, 0)
        assert _bits(ra) == _bits(rb)
        assert ra.stats.n_comparisons == rb.stats.n_comparisons > 0
        # appended after other games, and read back by the host backend
        a.clear()
        a.add_games([[0, 2]], [[1, 2]])
        assert a.add_completions(tr.ctx, learner, slots) == len(pl)
        b.clear()
        b.add_games([[0, 2]] + pl, [[1, 2]] + pc)
        assert _bits(a.fit(3, 0)) == _bits(b.fit(3, 0))
        assert _bits(a.fit(3, 0, backend="host")) == _bits(b.fit(3, 0, backend="host"))
        with pytest.raises(bppo.BppoError) as e:
            a.add_completions(tr.ctx, learner, [0, 1])          # the records name slot 2
        assert e.value.status == L.ERR_ARG and "slot" in str(e.value)
        assert _bits(a.fit(3, 0)) == _bits(b.fit(3, 0))        # and nothing was appended
    tr.close()


def test_add_completions_leaves_the_context_alone():
    out = []
    for call in (False, True):
        tr = _pool_ctx()
        bppo.collect_rollouts(tr.ctx)
        if call:
            with RatingTable() as t:
                assert t.add_completions(tr.ctx, 1, [0, 1, 2]) > 0
        _, m = bppo.train_step(tr.ctx, 1e-3, 0.01)
        out.append((tr.model.get_params().tobytes(), sorted((k, repr(v)) for k, v in m.items())))
        tr.close()
    assert out[0] == out[1]


# ---------------------------------------------------------------- Python layer ---
def test_rate_round_equals_compute_ratings():
    cfg = bppo.make_config("connect_four", num_envs=1, num_steps=4, hidden_size=64, num_hidden=2)
    params = [bppo.orthogonal_init(cfg, seed=11), bppo.orthogonal_init(cfg, seed=12), None]
    pods = [[0, 1], [2, 0]]
    rnd = bppo.run_round(cfg, params, [None] * 3, pods, 6, 8, bppo.TempSchedule(1.0), seeds=[5, 6])
    games = [(pod["contestants"], g) for pod in rnd for g in pod["games"]]
    assert len(games) == 12
    anchor = bppo.find_anchor_index(["step_00000200", "step_00000100", "Random"])
    assert anchor == 2
    a = bppo.rate_round(rnd, 3, anchor)
    b = compute_ratings(3, games, anchor)
    assert _bits(a) == _bits(b) and a.stats.n_games == 12
    ref = pl_ref.compute_ratings(3, games, anchor)
    assert a.stats.iterations_used == ref.iterations_used
    np.testing.assert_allclose([r.rating for r in a.ratings], [r[0] for r in ref.ratings], rtol=0, atol=1e-9)


def test_pool_trainer_feeds_the_rating_history():
    from test_gpu_opp_completions import N_OPP, make_cfg

    class Counting(bppo.RatingHistory):
        seen = 0
        skipped = 0

        def record_rollout(self, ctx, slot_to_pool, pool):
            comps, dropped = ctx.opponent_completions()
            assert dropped == 0
            cur = self.current_checkpoint or "step_00000000"
            for c in comps:
                names = [pool.get_checkpoint_name(slot_to_pool[m]) for m in c["position_to_opponent"] if m >= 0]
                self.seen += 1
                self.skipped += all(n == cur for n in names)
            return super().record_rollout(ctx, slot_to_pool, pool)

    cfg = make_cfg("connect_four", 16)
    pool = bppo.OpponentPool(2, 0.1, 1.0, 3)
    for k in range(3):
        pool.add_checkpoint(f"step_{(k + 1) * 1000:08d}", (k + 1) * 1000, bppo.orthogonal_init(cfg, seed=200 + k))
    hist = Counting()
    pt = bppo.PoolTrainer(cfg, pool, N_OPP, params=bppo.orthogonal_init(cfg, seed=5), rating_history=hist)
    # the learner first plays under the name of the opponent every env is seated against: the
    # whole first rollout is games against itself, which are skipped (main.rs:779-782)
    first = pool.available[pool.current_opponents[0]]
    hist.on_checkpoint_saved(first.checkpoint_name, first.checkpoint_step)
    assert hist.compute_ratings() == dict(current_elo=1000.0, best_elo=1000.0, best_step=0, total_games=0)
    pt.step()
    pt.add_checkpoint("step_00004000", 4000)        # the learner's name from here on
    assert hist.current_checkpoint == "step_00004000"
    pt.step()
    r = hist.compute_ratings()
    assert hist.skipped > 0 and r["total_games"] == hist.seen - hist.skipped > 0
    assert np.isfinite(r["current_elo"]) and r["best_elo"] >= r["current_elo"]
    pt.close()
    hist.close()


# --------------------------------------------------------------- argument errors ---
def test_argument_errors():
    with RatingTable() as t:
        def bad(msg, fn):
            with pytest.raises(bppo.BppoError) as e:
                fn()
            assert e.value.status == L.ERR_ARG and msg in str(e.value), str(e.value)
        bad("P outside 1..6", lambda: t.add_games(np.zeros((1, 7), np.int32), np.ones((1, 7), np.int32)))
        bad("placement < 1", lambda: t.add_games([[0, 1]], [[1, 0]]))
        bad("weight", lambda: t.add_games([[0, 1]], [[1, 2]], [0.0]))
        bad("weight", lambda: t.add_games([[0, 1]], [[1, 2]], [float("nan")]))
        bad("after a -1", lambda: t.add_games(np.array([[0, -1, 2]], np.int32), np.ones((1, 3), np.int32)))
        assert t.num_games == 0
        t.add_games([[0, 5]], [[1, 2]])
        bad("anchor outside", lambda: t.fit(6, 6))
        bad("anchor outside", lambda: t.fit(6, -1))
        bad(">= num_players", lambda: t.fit(5, 0))
        bad("num_players > 1024", lambda: t.fit(1025, 0))
        assert t.fit(6, 0).stats.n_games == 1
    with RatingTable(device=None) as h:
        h.add_games([[0, 1]], [[1, 2]])
        with pytest.raises(bppo.BppoError) as e:
            h.fit(2, 0, backend="device")
        assert e.value.status == L.ERR_ARG and "host-only" in str(e.value)
