"""CPU only: how often the solver's branches are taken on the sample of tests/test_gpu_solver_trim.py, counted with the float32 oracle.

The sample: rodent_optimized, 64 envs -- 48 states in contact after 30 env steps with seeded U(-1, 1) actions and 16 reset states
(qacc_warmstart = 0) -- stepped by 1 and by 10 substeps, CG and Newton, iteration caps 1, 2 and 8.  For the LAST substep of each case
(the one the debug dump describes) it prints how many envs left the solver loop at the cap and how many on a tolerance test
(solver_niter < cap), and how many started from qacc_smooth: the start is what a forward pass with 0 iterations leaves in
qacc_warmstart.  With --passes N it also prints the mean iterations per forward pass over N env steps at CG 8/8.

usage: python tools/solver_trim_sample.py [--passes N]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "brax-rodent-run_amd"))
import numpy as np

from oracle import ref
from rodent_amd import jax_random
from tests import util
from tests.oracle_env import OracleRodent

MODEL, N, N_RESET, WARM_STEPS = "rodent_optimized", 64, 16, 30


def sample():
    track = util.synthetic_track()
    A = OracleRodent(MODEL, N, "f32", (8, 8), track)
    A.reset(jax_random.split(jax_random.PRNGKey(11), N))
    first = A.b.state()
    rng = np.random.default_rng(7)
    for _ in range(WARM_STEPS):
        A.step(rng.uniform(-1, 1, (N, A.M.nu)).astype(np.float32))
    st = A.b.state()
    for k in st:
        st[k][N - N_RESET:] = first[k][N - N_RESET:]
    st["qacc_warmstart"][N - N_RESET:] = 0.0      # the state a reset hands to the first step
    return A, st, rng.uniform(-1, 1, (N, A.M.nu)).astype(np.float32)


def last_substep(A, st, ctrl, solver, cap, n_frames):
    """(niter, started from qacc_smooth) per env for the last of n_frames substeps."""
    M, b = A.M, A.b
    M.set_solver(solver)
    M.set_iterations(cap, 8)
    b.set_state(st)
    if n_frames > 1:
        ref.step_batch(M, b.d, ctrl, n_frames - 1)
    before = b.state()
    ref.step_batch(M, b.d, ctrl, 1)
    niter = b.get("solver_niter")[:, 0].astype(int)
    M.set_iterations(0, 8)
    b.set_state(before)
    ref.step_batch(M, b.d, ctrl, 1)
    start, smooth_at = b.get("qacc_warmstart"), b.get("qacc_smooth")
    M.set_iterations(8, 8)
    M.set_solver("cg")
    return niter, (start == smooth_at).all(1) & ~(start == before["qacc_warmstart"]).all(1)


if __name__ == "__main__":
    A, st, ctrl = sample()
    print("%s, %d envs (%d in contact after %d env steps, %d reset states), float32 oracle, last substep of each launch" % (MODEL, N, N - N_RESET, WARM_STEPS, N_RESET))
    print("solver cap substeps | ended at cap | on a tolerance | started at qacc_smooth | at qacc_warmstart")
    for solver in ("cg", "newton"):
        tot = np.zeros(4, int)
        for cap in (1, 2, 8):
            for nf in (1, 10):
                niter, smooth = last_substep(A, st, ctrl, solver, cap, nf)
                row = np.array([(niter >= cap).sum(), (niter < cap).sum(), smooth.sum(), (~smooth).sum()])
                tot += row
                print("%-6s %3d %8d | %12d | %14d | %22d | %17d" % ((solver, cap, nf) + tuple(row)))
        print("%-6s all          | %12d | %14d | %22d | %17d" % ((solver,) + tuple(tot)))
    if "--passes" in sys.argv:
        steps = int(sys.argv[sys.argv.index("--passes") + 1])
        A.b.set_state(st)
        A.b.sig_reset()
        rng = np.random.default_rng(3)
        for _ in range(steps):
            ref.step_batch(A.M, A.b.d, rng.uniform(-1, 1, (N, A.M.nu)).astype(np.float32), 10)
        sig = np.array(A.b.sigs(), dtype=np.float64)
        print("CG 8/8: %d forward passes, mean %.2f iterations per pass" % (sig[:, 3].sum(), sig[:, 2].sum() / sig[:, 3].sum()))
