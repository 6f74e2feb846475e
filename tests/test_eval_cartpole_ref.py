"""Single-player stats mode on the CPU alone: EvalStats.reward_summary against the numbers of
print_single_player_summary (eval.rs:416-469), the CartPole route of bppo.evaluate, and, for
every case test_gpu_eval_cartpole.py compares on the device, the preconditions that make the
case mean something, pinned on the Python restatement (tests/eval_ref_cartpole.py)."""
import inspect
import math

import pytest

import eval_ref_cartpole as X


def _stats(rewards, lengths):
    import bppo
    st = bppo.EvalStats(1)
    for r, n in zip(rewards, lengths):
        st.record_with_rewards([1], [r], n)
    return st


def test_reward_summary_matches_the_reference_numbers():
    s = _stats([100.0, 200.0, 150.0], [100, 200, 150]).reward_summary()
    assert s["mean"] == 150.0 and s["std"] == math.sqrt(5000.0 / 3.0)
    assert (s["min"], s["max"]) == (100.0, 200.0)
    assert (s["p25"], s["p50"], s["p75"]) == (100.0, 150.0, 200.0)       # sorted[3 * q / 100]
    assert (s["length_mean"], s["length_min"], s["length_max"]) == (150.0, 100, 200)


def test_reward_summary_percentile_index_and_empty():
    import bppo
    assert bppo.EvalStats(1).reward_summary() is None
    s = _stats([float(v) for v in (5, 1, 4, 2, 3, 8, 7, 6)], [1] * 8).reward_summary()
    assert (s["p25"], s["p50"], s["p75"]) == (3.0, 5.0, 7.0)            # sorted[2], [4], [6]
    s = _stats([9.0], [3]).reward_summary()
    assert (s["mean"], s["std"], s["p25"], s["p75"], s["length_max"]) == (9.0, 0.0, 9.0, 9.0, 3)


def test_evaluate_cartpole_needs_the_one_seat():
    import bppo
    cfg = X.net_config(16, 1, "relu")
    p = X.random_net(16, 1, "relu", 1)
    for seats in ([1], [0, 0], []):
        with pytest.raises(ValueError, match="seat_model"):
            bppo.evaluate(cfg, [p], None, seats, 5)


def test_python_surface_signatures():
    import bppo
    from bppo.eval import evaluate_episodes_ctx
    assert list(inspect.signature(evaluate_episodes_ctx).parameters) == [
        "ctx", "models", "normalizers", "num_games", "envs_per_pod", "temp_schedule", "seeds", "max_steps",
        "steps_per_launch"]
    assert list(inspect.signature(bppo.evaluate_episodes).parameters)[:9] == [
        "config", "models", "normalizers", "num_games", "envs_per_pod", "temp_schedule", "seeds", "seed", "device"]
    assert list(inspect.signature(bppo.evaluate_checkpoints).parameters)[:3] == ["dirs", "num_games", "envs_per_pod"]
    ts = bppo.TempSchedule.env_default("cartpole")                       # the trait default: 0.3 constant
    assert (float(ts.initial), ts.cutoff) == (float(X.f32(0.3)), None)


def _games_per_step(out):
    n = {}
    for g in out["games"]:
        n[g[5]] = n.get(g[5], 0) + 1
    return n


@pytest.mark.parametrize("name", list(X.CASES))
def test_case_preconditions(name):
    E, games = X.CASES[name][6], X.CASES[name][7]
    out = X.reference(name)
    assert out["ended_by"] == "num_games" and len(out["games"]) == games
    assert out["steps"] * 2 < X.MAX_STEPS
    assert max(_games_per_step(out).values()) >= 2          # some step records two or more episodes
    assert out["rng_pos"] == 2 + out["draws"]
    assert all(g[1][0] == 1 and g[4] == 0 for g in out["games"])
    if name in ("greedy", "greedy_zero", "truncation"):
        assert out["draws"] == 0 and out["rng_pos"] == 2
    else:
        assert out["draws"] > 0
    if name == "greedy_zero":                                # equal logits: the last maximum, always action 1
        assert max(g[2] for g in out["games"]) <= 12         # a constant push never balances
    if name == "cutoff":
        assert any(d > 0 and n > 0 for d, n in out["draws_per_step"])
        assert any(d == 0 and n > 0 for d, n in out["draws_per_step"])
    if name == "normalized_count1":                          # count < 2: the normalizer is not applied
        raw = X.run_reference(X.O.mlp_desc(5, 2, 16, 1, relu=False), X.case_model(X.CASES[name])[0], None, E, games,
                              X.CASES[name][8], X.CASES[name][9], X.MAX_STEPS)
        assert raw["games"] == out["games"] and raw["rng_pos"] == out["rng_pos"]
        assert X.reference("normalized")["games"] != out["games"]
    if name == "freeze":
        assert len(out["games"]) < E
        assert sorted(g[3] for g in out["games"]) == list(range(E - games, E))   # envs 0..10 frozen after step 0
    if name == "many_per_thread":
        assert E > 4 * 256 and len({g[3] for g in out["games"]}) > 256           # five envs per thread
    if name == "truncation":
        assert all(g[2] == 500 for g in out["games"]) and out["steps"] == 1000
        assert all(float(g[0][0]) == 500.0 for g in out["games"])


@pytest.mark.parametrize("shape", X.POD_SHAPES)
def test_pod_preconditions(shape):
    outs = [X.pod_reference(shape, k) for k in range(X.N_PODS)]
    for out in outs:
        assert out["ended_by"] == "num_games" and len(out["games"]) == X.POD_GAMES
        assert out["steps"] * 2 < X.MAX_STEPS and out["draws"] > 0
    assert max(max(_games_per_step(o).values()) for o in outs) >= 2
    assert len({o["rng_pos"] for o in outs}) > 1 and len({o["steps"] for o in outs}) > 1     # the pods differ
