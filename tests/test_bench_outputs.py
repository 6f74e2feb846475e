"""bench.py's options around the timed steps: a plain run asks for none of the extras
that take runs of their own (--full does), and --dump-outputs writes what the timed path
left after its last update, the same from run to run."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_lean_and_full_is_opt_in(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"
    # the older switches still parse, so the scripts that pass them keep working
    a = _parse(monkeypatch, "--no-cpu-baseline", "--no-learning", "--no-gae-isolated")
    assert not a.full


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def _run_and_dump(path, steps):
    import bppo
    cfg = bppo.make_config("cartpole", num_envs=256, num_steps=32)
    tr = bppo.Trainer(cfg, device=0, init_seed=0)
    try:
        mets, _ = tr.train_updates(steps)
        names = bench.dump_outputs(str(path), tr, mets[-1], 0)
        held = {"params": tr.model.get_params(), "advantages": tr.buffer.advantages.reshape(-1),
                "observations": tr.buffer.observations.reshape(-1, tr.ctx.obs_dim), "actions": tr.buffer.actions.reshape(-1)}
    finally:
        tr.close()
    return names, {n: np.load(os.path.join(str(path), n + ".npy")) for n in names}, held, mets[-1]


@pytest.mark.gpu
def test_dump_outputs_holds_the_last_update(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE_ROWS", 1000)       # 8192 rows: the sampling path
    names, got, held, last = _run_and_dump(tmp_path / "a", 2)
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in names)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) < 64 << 20
    rows = got["rollout_rows"].astype(np.int64)
    assert rows.size == 1000 and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 8192
    assert np.array_equal(got["params"], held["params"])
    assert np.array_equal(got["advantages"], held["advantages"][rows])
    assert np.array_equal(got["observations"], held["observations"][rows])
    assert np.array_equal(got["actions"], held["actions"][rows].astype(np.float32))
    m = dict(zip(bench.DUMP_METRICS, got["metrics"]))
    assert m["policy_loss"] == np.float64(last["policy_loss"]) and m["rng_word_pos"] == last["rng_word_pos"]
    assert m["num_updates"] == last["num_updates"] > 0
    # identical arguments -> identical inputs -> the same outputs, array for array
    _, again, _, _ = _run_and_dump(tmp_path / "b", 2)
    for n in names:
        assert np.array_equal(got[n], again[n], equal_nan=True), n
    # small buffers are written whole
    monkeypatch.setattr(bench, "DUMP_SAMPLE_ROWS", 8192)
    _, whole, held, _ = _run_and_dump(tmp_path / "c", 1)
    assert np.array_equal(whole["rollout_rows"], np.arange(8192))
    assert np.array_equal(whole["returns"].shape, (8192,))
