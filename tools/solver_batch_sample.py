"""CPU only: contacts in penetration per env on the sample of tests/test_gpu_solver_batch.py, counted with the float32 oracle.

The sample is tools/solver_trim_sample.py's (rodent_optimized, 64 envs: 48 in contact, 16 reset states), stepped by 1 and by 10 substeps,
CG and Newton, iteration caps 1 and 8.  For the LAST substep of each launch (the one the debug dump describes) it prints how many envs
fall in each piece class of the kernel's J*x jobs (Wave::contact_jobs: <= 16 contacts in penetration -> 4 lanes per contact, <= 32 -> 2,
more -> 1; 0 contacts is listed apart), and how many envs have any contact in penetration.  The test asserts the classes listed here.

usage: python tools/solver_batch_sample.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "brax-rodent-run_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from oracle import ref
import solver_trim_sample

CASES = [(solver, cap, nf) for solver in ("cg", "newton") for cap in (1, 8) for nf in (1, 10)]


def piece_classes(n_act):
    """Envs per class: (no contact, 1..16, 17..32, more than 32 contacts in penetration)."""
    n_act = np.asarray(n_act)
    return (int((n_act == 0).sum()), int(((n_act >= 1) & (n_act <= 16)).sum()), int(((n_act > 16) & (n_act <= 32)).sum()), int((n_act > 32).sum()))


def contacts_in_last_substep(A, st, ctrl, solver, cap, n_frames):
    M, b = A.M, A.b
    M.set_solver(solver)
    M.set_iterations(cap, 8)
    b.set_state(st)
    ref.step_batch(M, b.d, ctrl, n_frames)
    dist = b.get("con_dist")
    M.set_iterations(8, 8)
    M.set_solver("cg")
    return (dist < 0).sum(1)


if __name__ == "__main__":
    A, st, ctrl = solver_trim_sample.sample()
    print("%s, %d envs, float32 oracle, last substep of each launch" % (solver_trim_sample.MODEL, solver_trim_sample.N))
    print("solver cap substeps | envs in contact | no contact | 1..16 | 17..32 | > 32 | most contacts in one env")
    for solver, cap, nf in CASES:
        n_act = contacts_in_last_substep(A, st, ctrl, solver, cap, nf)
        print("%-6s %3d %8d | %15d | %10d | %5d | %6d | %4d | %d" % ((solver, cap, nf, int((n_act > 0).sum())) + piece_classes(n_act) + (int(n_act.max()),)))
