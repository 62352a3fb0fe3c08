"""The solver setup done once per substep (rr_kernel.h RR_LS_STAGE_ONCE): the line search's compacted row positions, its row count and its
D values are formed and staged once per substep instead of in every line search, and that must not change a bit of anything the kernel
writes.  The debug-dump instance can form and stage them in every line search, as before (`Batch.set_solver_batch(False)`).  (The solve-job
descriptors held in registers for the substep, RR_JOBS_RESIDENT, have no second path: the production instances carry them, and the
parity tests and the benchmark's output dumps cover them.)

The sample is tools/solver_trim_sample.py's: 48 states in contact after 30 env steps of seeded random actions and 16 reset states
(qacc_warmstart = 0).  tools/solver_batch_sample.py counts, with the float32 oracle on the CPU, the contacts in penetration in the last
substep of every launch below: every launch has 47 to 58 envs with 1 to 16 contacts (4 lanes per contact in Wave::contact_jobs), the
launch of CG with cap 1 over 10 substeps also 2 envs with 17 to 32 (2 lanes per contact, at most 20), and none has more than 32
(profiles/r13_g_solver_batch_sample.txt) -- so the first class is asserted per launch, the second for that launch, the third not at all."""
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
MID_CLASS_LAUNCH = ("cg", 1, 10)      # the launch where the oracle finds envs with 17 to 32 contacts in penetration


@pytest.fixture(scope="module")
def sample():
    """The CPU-chosen states (float32 oracle) and the action of the step that follows, on the device."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import solver_trim_sample
    assert (solver_trim_sample.MODEL, solver_trim_sample.N) == (MODEL, N)
    _, st, ctrl = solver_trim_sample.sample()
    dev = torch.device("cuda:0")
    return {k: torch.tensor(st[k], dtype=torch.float32, device=dev) for k in STATE}, torch.tensor(ctrl, dtype=torch.float32, device=dev)


def _debug_launch(solver, cap, n_frames, st, ctrl, batched):
    """One launch of `n_frames` substeps of the debug-dump instance: state, dump and work estimate as int32 bit patterns, and the dump as numbers."""
    from rodent_amd import assets, hip
    dev = torch.device("cuda:0")
    batch = hip.Batch(hip.Model(assets.asset_path(MODEL), cap, LS_ITER, solver=solver), N, dev)
    lay = batch.debug_layout()
    dbg = torch.zeros(N, batch.dims.dbg_floats, device=dev)
    cost = torch.zeros(N, dtype=torch.int32, device=dev)
    batch.set_schedule(None, cost)
    batch.set_solver_batch(batched)
    s = {k: v.clone() for k, v in st.items()}
    batch.pipeline_step(s, ctrl, n_frames, out=dict(debug=dbg))
    torch.cuda.synchronize()
    out = {k: v.view(torch.int32).cpu().numpy() for k, v in s.items()}
    out["cost"] = cost.cpu().numpy()
    d = dbg.view(torch.int32).cpu().numpy()
    for name, (o, n) in lay.items():
        out["dump:" + name] = d[:, o:o + n]
    num = dbg.cpu().numpy()
    return out, {name: num[:, o:o + n] for name, (o, n) in lay.items()}


@pytest.fixture(scope="module")
def launches(sample):
    """{(solver, cap, substeps): (unbatched, batched)}: every launch once, shared by the tests below."""
    st, ctrl = sample
    return {(solver, cap, nf): (_debug_launch(solver, cap, nf, st, ctrl, False), _debug_launch(solver, cap, nf, st, ctrl, True))
            for solver in ("cg", "newton") for cap in CAPS for nf in FRAMES}


def _classes(dump):
    """Contacts in penetration per env in the dumped (last) substep, and the envs per piece class of Wave::contact_jobs."""
    n_act = (dump["con_dist"] < 0).sum(1)
    return n_act, (int(((n_act >= 1) & (n_act <= 16)).sum()), int(((n_act > 16) & (n_act <= 32)).sum()), int((n_act > 32).sum()))


@pytest.mark.parametrize("n_frames", FRAMES)
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_batched_equals_unbatched(launches, solver, cap, n_frames):
    """Every dumped array (niter, cost, ls_iters and solver_end among them), the four state arrays and the work estimate are bitwise equal."""
    (off, _), (on, dump) = launches[(solver, cap, n_frames)]
    n_act, cls = _classes(dump)
    niter = dump["niter_cost"][:, 0].astype(int)
    print(solver, "cap", cap, "substeps", n_frames, "| envs in contact", int((n_act > 0).sum()), "| envs with <= 16 / <= 32 / > 32 contacts in penetration", cls,
          "| most", int(n_act.max()), "| smooth start", int(dump["solver_end"][:, 0].sum()), "| niter max", int(niter.max()))
    assert set(off) == set(on) and len(off) > 20
    assert int((on["dump:kernarg_ok"] != 0).all()) and int((off["dump:kernarg_ok"] != 0).all())
    differing = [k for k in off if not np.array_equal(off[k], on[k])]
    assert not differing, differing
    assert (on["cost"] > 0).any()
    assert np.isfinite(on["qpos"].view(np.float32)).all()
    # not vacuous: contacts are walked, and in the piece classes the oracle finds in this launch
    assert int((n_act > 0).sum()) >= 16
    assert cls[0] >= 16
    if (solver, cap, n_frames) == MID_CLASS_LAUNCH:
        assert cls[1] >= 1


@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_both_starts_and_several_iterations_are_in_the_sample(launches, solver):
    """Both warm-start candidates are chosen somewhere, and some last substep runs at least two iterations: the values staged once serve
    more than one line search."""
    ends = np.concatenate([launches[(solver, cap, nf)][1][1]["solver_end"] for cap in CAPS for nf in FRAMES]).astype(int)
    niter = np.concatenate([launches[(solver, 8, nf)][1][1]["niter_cost"][:, 0] for nf in FRAMES]).astype(int)
    smooth, warm = int((ends[:, 0] == 1).sum()), int((ends[:, 0] == 0).sum())
    print(solver, "last substeps: smooth start", smooth, "warm start", warm, "| at cap 8: envs with >= 2 iterations", int((niter >= 2).sum()))
    assert smooth >= 8 and warm >= 16
    assert int((niter >= 2).sum()) >= 1
