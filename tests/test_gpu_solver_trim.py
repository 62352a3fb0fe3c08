"""The trimmed solver (rr_kernel.h Wave::solve): the exit test made before the solve for Mgrad, the cost-only context at qacc_smooth
without its contact walk, and that context's rows reused where it is chosen must not change a bit of anything the kernel writes.
The debug-dump instance can do all of that work anyway, in the reference's order (`Batch.set_solver_trim(False)`), and dumps for the
last substep which start was chosen and how the loop ended (dump field `solver_end`).

The sample is the one tools/solver_trim_sample.py counts on the CPU with the float32 oracle: 48 states in contact after 30 env steps
of seeded random actions and 16 reset states (qacc_warmstart = 0).  There, over the twelve launches per solver below, 333 (CG) / 233
(Newton) last substeps end at the cap and 51 / 151 on a tolerance test, 83 / 101 start from qacc_smooth and 301 / 283 from
qacc_warmstart (profiles/r12_g_solver_trim_sample.txt); a cap of 1 never ends on a tolerance and Newton never reaches a cap of 8, so the branch counts are asserted per solver."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL, N, LS_ITER = "rodent_optimized", 64, 8
CAPS, FRAMES = (1, 2, 8), (1, 10)
STATE = ("qpos", "qvel", "act", "qacc_warmstart")


@pytest.fixture(scope="module")
def sample():
    """The CPU-chosen states (float32 oracle) and the action of the step that follows, on the device."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import solver_trim_sample
    assert (solver_trim_sample.MODEL, solver_trim_sample.N) == (MODEL, N)
    _, st, ctrl = solver_trim_sample.sample()
    dev = torch.device("cuda:0")
    assert not st["qacc_warmstart"][N - solver_trim_sample.N_RESET:].any() and st["qacc_warmstart"][:N - solver_trim_sample.N_RESET].any()
    return {k: torch.tensor(st[k], dtype=torch.float32, device=dev) for k in STATE}, torch.tensor(ctrl, dtype=torch.float32, device=dev)


def _debug_launch(solver, cap, n_frames, st, ctrl, trim):
    """One launch of `n_frames` substeps of the debug-dump instance (the single-step form): state, dump and work estimate as int32 bit patterns; `solver_end` as numbers."""
    from rodent_amd import assets, hip
    dev = torch.device("cuda:0")
    batch = hip.Batch(hip.Model(assets.asset_path(MODEL), cap, LS_ITER, solver=solver), N, dev)
    lay = batch.debug_layout()
    dbg = torch.zeros(N, batch.dims.dbg_floats, device=dev)
    cost = torch.zeros(N, dtype=torch.int32, device=dev)
    batch.set_schedule(None, cost)
    batch.set_solver_trim(trim)
    s = {k: v.clone() for k, v in st.items()}
    batch.pipeline_step(s, ctrl, n_frames, out=dict(debug=dbg))
    torch.cuda.synchronize()
    out = {k: v.view(torch.int32).cpu().numpy() for k, v in s.items()}
    out["cost"] = cost.cpu().numpy()
    d = dbg.view(torch.int32).cpu().numpy()
    for name, (o, n) in lay.items():
        out["dump:" + name] = d[:, o:o + n]
    o, n = lay["solver_end"]
    o2, _ = lay["niter_cost"]
    return out, dbg[:, o:o + n].cpu().numpy().astype(int), dbg[:, o2].cpu().numpy().astype(int), lay


@pytest.fixture(scope="module")
def launches(sample):
    """{(solver, cap, substeps): (untrimmed, trimmed)}: every launch once, shared by the tests below."""
    st, ctrl = sample
    return {(solver, cap, nf): (_debug_launch(solver, cap, nf, st, ctrl, False), _debug_launch(solver, cap, nf, st, ctrl, True))
            for solver in ("cg", "newton") for cap in CAPS for nf in FRAMES}


@pytest.mark.parametrize("n_frames", FRAMES)
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_trimmed_equals_untrimmed(launches, solver, cap, n_frames):
    """Every dumped array (niter, cost and solver_end among them), the four state arrays and the work estimate are bitwise equal."""
    (off, _, _, _), (on, end, niter, _) = launches[(solver, cap, n_frames)]
    print(solver, "cap", cap, "substeps", n_frames, "| smooth start", int(end[:, 0].sum()), "| ended: cap", int((end[:, 1] & 1 != 0).sum()),
          "improvement", int((end[:, 1] & 2 != 0).sum()), "gradient", int((end[:, 1] & 4 != 0).sum()))
    assert set(off) == set(on) and len(off) > 20
    assert int((on["dump:kernarg_ok"] != 0).all()) and int((off["dump:kernarg_ok"] != 0).all())
    differing = [k for k in off if not np.array_equal(off[k], on[k])]
    assert not differing, differing
    assert (on["cost"] > 0).any()
    assert np.isfinite(on["qpos"].view(np.float32)).all()
    # the dump is consistent with itself: some test ended the loop, the cap bit is niter == cap, nobody ran past the cap
    assert (end[:, 1] != 0).all() and (end[:, 1] < 8).all() and set(np.unique(end[:, 0])) <= {0, 1}
    assert np.array_equal(end[:, 1] & 1 != 0, niter == cap) and (niter <= cap).all()


@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_every_branch_is_in_the_sample(launches, solver):
    """Both starts and both kinds of exit occur, with and without the trim alike (the dumps are equal), so the identity above is not vacuous."""
    ends = np.concatenate([launches[(solver, cap, nf)][1][1] for cap in CAPS for nf in FRAMES])
    at_cap, on_tol = int((ends[:, 1] & 1 != 0).sum()), int((ends[:, 1] & 1 == 0).sum())
    smooth, warm = int((ends[:, 0] == 1).sum()), int((ends[:, 0] == 0).sum())
    print(solver, "last substeps: ended at cap", at_cap, "on a tolerance alone", on_tol, "| smooth start", smooth, "warm start", warm)
    assert at_cap >= 16 and on_tol >= 16
    assert smooth >= 8 and warm >= 16
    # each tolerance test ends some loop (which of the two fires is not told by the oracle, so: taken at all)
    assert int((ends[:, 1] & 2 != 0).sum()) > 0 and int((ends[:, 1] & 4 != 0).sum()) > 0


def test_dump_layout(launches):
    lay = launches[("cg", 8, 1)][1][3]
    assert lay["solver_end"][1] == 2
    assert lay["solver_end"][0] == lay["ls_iters"][0] + lay["ls_iters"][1]      # behind ls_iters, before kernarg_ok
