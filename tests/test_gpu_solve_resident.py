"""The inverse factor's entries held in registers for the substep (rr_kernel.h RR_SOLVE_MAT_RESIDENT): the undamped M^-1 solves of the
fixed-dimension instances multiply this lane's entries of W from registers, read once after the inversion, instead of gathering them from
LDS in every solve -- and that must not change a bit of anything the kernel writes.  `Batch.set_solve_resident(False)` runs the same
production single-step instance built with the entries left in LDS (rr_matlds_kernel), so the two can be compared in one library.

The sample is tools/solver_trim_sample.py's: 48 states in contact after 30 env steps of seeded random actions and 16 reset states
(qacc_warmstart = 0); profiles/r13_g_solver_batch_sample.txt records 47 to 58 envs in contact in the last substep of these launches.  One
launch of the debug-dump instance per case shows that the solves are exercised: contacts in penetration (a solver that iterates: one
solve per CG iteration) and, at cap 8, envs with two iterations or more."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL, N, LS_ITER = "rodent_optimized", 64, 8
CAPS, FRAMES = (1, 8), (1, 10)
STATE = ("qpos", "qvel", "act", "qacc_warmstart")


@pytest.fixture(scope="module")
def sample():
    """The CPU-chosen states (float32 oracle) and the action of the step that follows, on the device."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import solver_trim_sample
    assert (solver_trim_sample.MODEL, solver_trim_sample.N) == (MODEL, N)
    _, st, ctrl = solver_trim_sample.sample()
    dev = torch.device("cuda:0")
    return {k: torch.tensor(st[k], dtype=torch.float32, device=dev) for k in STATE}, torch.tensor(ctrl, dtype=torch.float32, device=dev)


def _env_launch(cap, n_frames, st, ctrl, resident):
    """One env step of `n_frames` substeps through the production single-step instance: everything it writes, as int32 bit patterns."""
    from rodent_amd import assets, hip
    from tests import util
    dev = torch.device("cuda:0")
    batch = hip.Batch(hip.Model(assets.asset_path(MODEL), cap, LS_ITER, solver="cg"), N, dev)
    cost = torch.zeros(N, dtype=torch.int32, device=dev)
    batch.set_schedule(None, cost)
    batch.set_solve_resident(resident)
    env = dict(track_pos=torch.tensor(util.synthetic_track(), dtype=torch.float32, device=dev), cur_frame=torch.zeros(N, dtype=torch.int32, device=dev),
               obs=torch.zeros(N, batch.dims.obs_dim, device=dev), reward=torch.zeros(N, device=dev), done=torch.zeros(N, device=dev),
               metrics=torch.zeros(N, 3, device=dev))
    s = {k: v.clone() for k, v in st.items()}
    batch.env_step(s, ctrl, n_frames, env)
    torch.cuda.synchronize()
    out = {k: v.view(torch.int32).cpu().numpy() for k, v in s.items()}
    for k in ("obs", "reward", "done", "metrics"):
        out[k] = env[k].view(torch.int32).cpu().numpy()
    out["work"] = cost.cpu().numpy()
    return out


def _debug_dump(cap, n_frames, st, ctrl):
    """The same substeps through the debug-dump instance: the dump of the last one, as numbers."""
    from rodent_amd import assets, hip
    dev = torch.device("cuda:0")
    batch = hip.Batch(hip.Model(assets.asset_path(MODEL), cap, LS_ITER, solver="cg"), N, dev)
    dbg = torch.zeros(N, batch.dims.dbg_floats, device=dev)
    batch.pipeline_step({k: v.clone() for k, v in st.items()}, ctrl, n_frames, out=dict(debug=dbg))
    torch.cuda.synchronize()
    num = dbg.cpu().numpy()
    return {name: num[:, o:o + n] for name, (o, n) in batch.debug_layout().items()}


@pytest.fixture(scope="module")
def launches(sample):
    """{(cap, substeps): (entries in LDS, entries resident, debug dump)}: every launch once, shared by the tests below."""
    st, ctrl = sample
    return {(cap, nf): (_env_launch(cap, nf, st, ctrl, False), _env_launch(cap, nf, st, ctrl, True), _debug_dump(cap, nf, st, ctrl))
            for cap in CAPS for nf in FRAMES}


@pytest.mark.parametrize("n_frames", FRAMES)
@pytest.mark.parametrize("cap", CAPS)
def test_resident_equals_lds(launches, cap, n_frames):
    """qpos, qvel, act, qacc_warmstart, obs, reward, done, metrics and the work estimate are bitwise equal, on a launch whose solver runs."""
    off, on, dump = launches[(cap, n_frames)]
    n_act = (dump["con_dist"] < 0).sum(1)
    niter = dump["niter_cost"][:, 0].astype(int)
    print("cap", cap, "substeps", n_frames, "| envs with a contact in penetration", int((n_act > 0).sum()), "| niter max", int(niter.max()),
          "| envs with >= 2 iterations", int((niter >= 2).sum()))
    assert set(off) == set(on) == set(STATE) | {"obs", "reward", "done", "metrics", "work"}
    differing = [k for k in off if not np.array_equal(off[k], on[k])]
    assert not differing, differing
    assert np.isfinite(on["qpos"].view(np.float32)).all() and np.isfinite(on["obs"].view(np.float32)).all()
    assert (on["work"] > 0).any()
    # not vacuous: the launch exercises the solves
    assert int((dump["kernarg_ok"] != 0).all())
    assert int((n_act > 0).sum()) >= 16


def test_some_env_runs_several_iterations_at_cap_8(launches):
    """At cap 8 some last substep runs at least two CG iterations: the resident entries serve more than one solve."""
    niter = np.concatenate([launches[(8, nf)][2]["niter_cost"][:, 0] for nf in FRAMES]).astype(int)
    print("cap 8: envs with >= 2 iterations", int((niter >= 2).sum()), "of", niter.size)
    assert int((niter >= 2).sum()) >= 1


def test_switch_refusals():
    """The switch is refused, in words, for a model of other dimensions, and a batch with the switch off refuses the launches it has no instance for."""
    from rodent_amd import assets, hip
    dev = torch.device("cuda:0")
    other = hip.Batch(hip.Model(assets.asset_path("rodent_new"), 8, LS_ITER, solver="cg"), 4, dev)
    with pytest.raises(RuntimeError, match="rr_batch_set_solve_resident: only the fixed-dimension CG instance of the rodent_optimized dimensions"):
        other.set_solve_resident(False)
    other.set_solve_resident(True)
    batch = hip.Batch(hip.Model(assets.asset_path(MODEL), 8, LS_ITER, solver="cg"), 4, dev)
    batch.set_solve_resident(False)
    dbg = torch.zeros(4, batch.dims.dbg_floats, device=dev)
    with pytest.raises(RuntimeError, match="serves production launches only"):
        batch.pipeline_step(batch.zeros_state(), torch.zeros(4, batch.dims.nu, device=dev), 1, out=dict(debug=dbg))
    torch.cuda.synchronize()
