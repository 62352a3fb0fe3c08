"""`bench.py --dump-outputs DIR` on the CPU: what is written (float32 / float64 only), the size cap with its fixed, seeded env sample,
and the arrays taken from an env state and from ppo.train's parameters."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rodent_amd.envs.base import PipelineState, State  # noqa: E402


def test_dtypes_and_names(tmp_path):
    arrays = {"obs": np.ones((4, 3), np.float32), "info.cur_frame": np.arange(4, dtype=np.int32), "done": np.array([True, False] * 2),
              "x64": np.zeros(2, np.float64)}
    bench.write_outputs(str(tmp_path), arrays, 4)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == set(arrays)
    assert got["obs"].dtype == np.float32 and got["x64"].dtype == np.float64
    assert got["info.cur_frame"].dtype == np.float64 and np.array_equal(got["info.cur_frame"], np.arange(4))
    assert np.array_equal(got["done"], [1, 0, 1, 0])


def test_size_cap_keeps_the_same_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1000 * 4 * 8 // 2)
    n = 1000
    arrays = {"a": np.arange(n * 4, dtype=np.float32).reshape(n, 4), "b": np.arange(n, dtype=np.float32), "w": np.ones(3, np.float32)}
    for d in ("one", "two"):
        bench.write_outputs(str(tmp_path / d), arrays, n)
    a1, b1, a2 = (np.load(tmp_path / p) for p in ("one/a.npy", "one/b.npy", "two/a.npy"))
    assert sum(os.path.getsize(tmp_path / "one" / f) - 128 for f in os.listdir(tmp_path / "one")) <= bench.DUMP_LIMIT_BYTES
    assert np.array_equal(a1, a2) and np.array_equal(a1[:, 0] / 4, b1)           # same rows in every array and every run
    assert np.all(np.diff(b1) > 0) and len(b1) < n
    assert np.array_equal(np.load(tmp_path / "one/w.npy"), np.ones(3))


def test_arrays_of_a_state_and_of_params():
    N = 5
    ps = PipelineState(qpos=torch.zeros(N, 7), qvel=torch.zeros(N, 6), act=torch.zeros(N, 0), qacc_warmstart=torch.zeros(N, 6))
    st = State(pipeline_state=ps, obs=torch.ones(N, 9), reward=torch.zeros(N), done=torch.zeros(N),
               metrics={"r": torch.ones(N)}, info={"steps": torch.ones(N), "first_obs": torch.ones(N, 9), "note": "x"})
    a = bench.state_arrays(st)
    assert set(a) == {"obs", "reward", "done", "qpos", "qvel", "act", "qacc_warmstart", "metrics.r", "info.steps"}
    net = torch.nn.Linear(3, 2)
    p = bench.params_arrays((None, net))
    assert set(p) == {"policy.weight", "policy.bias"} and p["policy.weight"].shape == (2, 3)
