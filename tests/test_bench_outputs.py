"""bench.py --dump-outputs: the files hold what the timed steps left for their
caller (the simulator's tensors after the last timed step, and the rollouts'
recorded rows), identical from run to run and however the steps are staged;
a plain run (no --full) carries none of the extra legs."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, WARMUP, STEPS, SEED = 96, 3, 12, 321


@pytest.fixture(scope="module", autouse=True)
def _libs(native_lib, oracle_lib):
    pass


def run_bench(monkeypatch, capsys, out_dir, *extra):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--exec", "cpu", "--worlds", str(W), "--steps",
                                      str(STEPS), "--warmup", str(WARMUP), "--dump-outputs", str(out_dir), *extra])
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def load(out_dir):
    return {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


@pytest.fixture(scope="module")
def expected():
    """The same steps on a simulator of the test's own: every column after the last one."""
    from madrona_basketball_amd import ExecMode
    from tests.helpers import make_sim
    sim = make_sim(ExecMode.CPU, W, per_world_rng=True)
    sim.step_n(WARMUP + STEPS, random_actions=True, action_seed=SEED, step0=0)
    return {k: v.numpy().copy() for k, v in sim.snapshot().items()}


def test_plain_run_dumps_the_last_steps_outputs(monkeypatch, capsys, tmp_path, expected):
    out = run_bench(monkeypatch, capsys, tmp_path / "a")
    assert out["steps"] == STEPS and out["ms_per_step"] > 0 and out["value"] > 0
    # a plain run times nothing but its steps
    assert out["roofline"] is None and out["cpu_baseline"] is None and out["cpu_executor"] is None
    assert not {"e2e", "per_call_step", "roofline_beyond_cache"} & set(out)
    got = load(tmp_path / "a")
    assert np.array_equal(got.pop("worlds"), np.arange(W))
    # the action tensor is the caller's input (the staged rows stand in for it)
    assert set(got) == set(expected)
    for k, a in got.items():
        assert a.dtype in (np.float32, np.float64), k
        if k == "action":
            continue
        e = expected[k]
        assert a.shape == e.shape, k
        if e.dtype == np.float32:
            assert np.array_equal(a.view(np.uint32), e.view(np.uint32)), k
        else:
            assert np.array_equal(a, e.astype(np.float64)), k
    assert sum(a.nbytes for a in got.values()) <= 64e6


def test_dump_is_the_same_staged_in_chunks(monkeypatch, capsys, tmp_path):
    """Steps staged and timed in several chunks (a long run) are the same steps."""
    import bench
    run_bench(monkeypatch, capsys, tmp_path / "one")
    monkeypatch.setattr(bench, "STAGE_MAX_BYTES", 5 * W * 2 * 24)  # 5 steps at a time: 5 + 5 + 2
    out = run_bench(monkeypatch, capsys, tmp_path / "chunks")
    assert out["steps"] == STEPS
    a, b = load(tmp_path / "one"), load(tmp_path / "chunks")
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_dump_samples_worlds_beyond_the_size_bound(monkeypatch, capsys, tmp_path):
    import bench
    run_bench(monkeypatch, capsys, tmp_path / "all", "--rollout", "4")
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 * 1024)
    run_bench(monkeypatch, capsys, tmp_path / "some", "--rollout", "4")
    full, part = load(tmp_path / "all"), load(tmp_path / "some")
    keep = part["worlds"].astype(np.int64)
    assert 0 < len(keep) < W and np.all(np.diff(keep) > 0)
    assert sum(a.nbytes for a in part.values()) <= 64 * 1024
    assert full["rollout_obs"].shape[:2] == (4, W)
    for k, a in part.items():
        if k != "worlds":
            axis = 1 if k.startswith("rollout_") else 0
            assert np.array_equal(a, np.take(full[k], keep, axis=axis), equal_nan=True), k
