"""The bad-state check (Rodent(bad_state_max=...); rr_env_io::bad_state_max) as far as it can be held without a GPU: the pure-torch
statement of the rule, the constructor's refusals, ppo.train's bookkeeping of the counter, and what the check did to the step kernel's
instances in the built code object (it is a run-time flag in the shared epilogue: no new instance, no scratch, no VGPR spill)."""
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from rodent_amd import hip
from rodent_amd.envs.rodent import Rodent, bad_state_mask
from rodent_amd.training.agents.ppo import train as ppo
from tests import util
from tests.fake_env import PointEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bad_state_mask_on_hand_made_rows():
    thr = 1e10
    t32 = np.float32(thr)
    up = float(np.nextafter(t32, np.float32(np.inf)))
    qpos = torch.zeros(9, 5)
    qvel = torch.zeros(9, 4)
    qpos[1, 3] = float("nan")
    qvel[2, 0] = float("inf")
    qpos[3, 4] = float("-inf")
    qvel[4, 1] = float(t32)             # exactly at the threshold: not bad
    qvel[5, 2] = up                     # the next float up: bad
    qpos[6, 0] = -up                    # ... in magnitude
    qpos[7, 1] = -float(t32)
    qvel[8, 3] = 1e12                   # finite and too large
    got = bad_state_mask(qpos, qvel, thr)
    assert got.dtype == torch.bool and got.shape == (9,)
    assert got.tolist() == [False, True, True, True, False, True, True, False, True]
    # a tightened threshold
    assert bad_state_mask(torch.tensor([[0.5, -2.0]]), torch.tensor([[1.0]]), 1.5).tolist() == [True]
    assert bad_state_mask(torch.tensor([[0.5, -1.5]]), torch.tensor([[1.0]]), 1.5).tolist() == [False]


@pytest.mark.parametrize("value", [0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"),
                                   1e-50, 1e39])      # float32 is what reaches the kernel: these two arrive there as 0 (= off) and inf
def test_constructor_refuses_thresholds_that_are_not_positive_and_finite(value):
    with pytest.raises(ValueError, match="bad_state_max"):
        Rodent(util.synthetic_track(), xml_path="rodent_optimized.xml", num_envs=2, device="cpu", bad_state_max=value)


class CountingPointEnv(PointEnv):
    """PointEnv with the two attributes ppo.train looks at; `bad_states()` answers from a script (the running total per call)."""

    def __init__(self, num_envs=8, device="cpu", bad_state_max=None, script=None, calls=None):
        super().__init__(num_envs, device)
        self.bad_state_max = bad_state_max
        self.script = script if script is not None else []
        self.calls = calls if calls is not None else []

    def with_num_envs(self, n, device=None):
        return CountingPointEnv(n, device or self.device, self.bad_state_max, self.script, self.calls)

    def bad_states(self):
        self.calls.append(len(self.calls))
        return self.script[len(self.calls) - 1]


def _train(env, steps_per_report, reports):
    log = []
    per_step = 16 * 4 * 2                 # batch_size * unroll_length * num_minibatches
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        ppo.train(environment=env, num_timesteps=per_step * steps_per_report * reports, episode_length=20, num_envs=16, batch_size=16,
                  num_minibatches=2, unroll_length=4, num_updates_per_batch=1, num_evals=reports + 1, num_eval_envs=0, seed=0,
                  progress_fn=lambda n, m: log.append(dict(m)))
    return log, [w for w in caught if "bad_state_max" in str(w.message)]


def test_train_reports_the_counter_as_a_difference_per_report_and_warns_once():
    # two training steps per report, three reports: the running totals the env answers with, one per training step
    env = CountingPointEnv(16, bad_state_max=1e10, script=[0, 0, 3, 5, 5, 9])
    log, warned = _train(env, 2, 3)
    assert len(env.calls) == 6 and len(log) == 3
    assert [m["training/bad_state_resets"] for m in log] == [0.0, 5.0, 4.0]
    assert len(warned) == 1 and issubclass(warned[0].category, RuntimeWarning) and "3 (env, step) events" in str(warned[0].message)


def test_train_reports_nothing_while_the_check_is_off():
    env = CountingPointEnv(16, bad_state_max=None, script=[7] * 8)
    log, warned = _train(env, 1, 2)
    assert len(log) == 2 and not env.calls and not warned
    assert all("training/bad_state_resets" not in m for m in log)
    # ... and an env without the method is left alone too
    log, warned = _train(PointEnv(16), 1, 2)
    assert all("training/bad_state_resets" not in m for m in log) and not warned


@pytest.fixture(scope="module")
def kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    return kernel_meta.kernels(hip.LIB_PATH)


def test_the_check_added_no_kernel_instance(kernels):
    """The check is a run-time flag in the epilogue all env-step instances share, so the code object holds the instances it held:
    23 of rr_step_kernel (22 when the check was added; the debug dump of the candidate-pair models came later), 9 of rr_rand_kernel,
    4 of rr_eval_kernel."""
    count = lambda stem: sum(k["name"].startswith("_Z14" + stem) for k in kernels)
    assert (count("rr_step_kernel"), count("rr_rand_kernel"), count("rr_eval_kernel")) == (23, 9, 4)


def test_every_instance_is_free_of_scratch_and_vgpr_spills(kernels):
    ks = [k for k in kernels if any(s in k["name"] for s in ("rr_step_kernel", "rr_rand_kernel", "rr_eval_kernel"))]
    assert len(ks) == 36
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (k["name"], k["scratch"], k["vgpr_spill"])


def test_abi_carries_the_threshold_and_the_counter():
    assert hip.RREnvIO._fields_[-1] == ("bad_state_max", hip.C.c_float)
    assert hip.C.sizeof(hip.RREnvIO) == 80            # the new member fills the struct's tail padding: its size is unchanged
    assert "rr_batch_bad_states" in hip.EXPORTS
    assert math.isclose(hip.RREnvIO(bad_state_max=0.0).bad_state_max, 0.0)
