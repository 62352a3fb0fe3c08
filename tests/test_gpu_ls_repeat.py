"""The line search's repeat exit (rr_kernel.h RR_LS_REPEAT_EXIT): leaving the bracketing loop after an iteration that left the
bracket bitwise unchanged must not change a bit of anything the kernel writes.  The debug-dump instance can run the repeated
iterations anyway (`Batch.set_ls_repeat_exit(False)`) and counts, per env and for the last substep, the bracketing iterations
it executed and those the exit left out (dump field `ls_iters`)."""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

MODEL, N, ITER, LS_ITER, N_FRAMES = "rodent_optimized", 16, 8, 8, 10
STATE = ("qpos", "qvel", "act", "qacc_warmstart")


@pytest.fixture(scope="module")
def states_in_contact():
    """States after 12 wrapped env steps with seeded U(-1, 1) actions on the production path, and the action of the step that follows."""
    from rodent_amd import envs, jax_random
    from rodent_amd.envs import wrappers
    dev = torch.device("cuda:0")
    env = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=N, xml_path=MODEL + ".xml",
                               iterations=ITER, ls_iterations=LS_ITER, device=dev)
    wenv = wrappers.wrap(env, episode_length=150, action_repeat=1)
    state = wenv.reset(jax_random.split(jax_random.PRNGKey(11), N))
    g = torch.Generator(device=dev).manual_seed(7)
    for _ in range(12):
        state = wenv.step(state, torch.rand(N, env.action_size, device=dev, generator=g) * 2 - 1)
    ctrl = torch.rand(N, env.action_size, device=dev, generator=g) * 2 - 1
    torch.cuda.synchronize()
    ps = state.pipeline_state
    return {k: getattr(ps, k).clone() for k in STATE}, ctrl


def _debug_launch(solver, st, ctrl, exit_on):
    """One single-step launch (one env step of 10 substeps) of the debug-dump instance: state, dump and work estimate as int32 bit patterns."""
    from rodent_amd import assets, hip
    dev = torch.device("cuda:0")
    batch = hip.Batch(hip.Model(assets.asset_path(MODEL), ITER, LS_ITER, solver=solver), N, dev)
    lay = batch.debug_layout()
    dbg = torch.zeros(N, batch.dims.dbg_floats, device=dev)
    cost = torch.zeros(N, dtype=torch.int32, device=dev)
    batch.set_schedule(None, cost)
    batch.set_ls_repeat_exit(exit_on)
    s = {k: v.clone() for k, v in st.items()}
    batch.pipeline_step(s, ctrl, N_FRAMES, out=dict(debug=dbg))
    torch.cuda.synchronize()
    out = {k: v.view(torch.int32).cpu().numpy() for k, v in s.items()}
    out["cost"] = cost.cpu().numpy()
    o, n = lay["ls_iters"]
    counts = dbg[:, o:o + n].cpu().numpy().astype(np.float64)
    d = dbg.view(torch.int32).cpu().numpy()
    for name, (o, n) in lay.items():
        if name != "ls_iters":
            out["dump:" + name] = d[:, o:o + n]
    return out, counts, lay


@pytest.mark.parametrize("solver", ["cg", "newton"])
def test_exit_on_equals_exit_off(states_in_contact, solver):
    """Every dumped array, the four state arrays and the work estimate are bitwise equal with the exit off and on; per env the
    iterations executed without the exit are those executed plus those left out with it; and the exit is taken at all."""
    st, ctrl = states_in_contact
    off, c_off, _ = _debug_launch(solver, st, ctrl, False)
    on, c_on, _ = _debug_launch(solver, st, ctrl, True)
    print(solver, "bracketing iterations of the last substep per env: exit off", c_off[:, 0].astype(int).tolist(),
          "| exit on: executed", c_on[:, 0].astype(int).tolist(), "left out", c_on[:, 1].astype(int).tolist())
    assert set(off) == set(on) and len(off) > 20
    assert int((on["dump:kernarg_ok"] != 0).all())
    differing = [k for k in off if not np.array_equal(off[k], on[k])]
    assert not differing, differing
    assert (on["cost"] > 0).any()
    assert np.array_equal(c_off[:, 1], np.zeros(N))
    assert np.array_equal(c_off[:, 0], c_on[:, 0] + c_on[:, 1])
    assert c_on[:, 1].sum() > 0


def test_dump_layout_and_count_range(states_in_contact):
    st, ctrl = states_in_contact
    _, counts, lay = _debug_launch("cg", st, ctrl, True)
    assert lay["ls_iters"][1] == 2
    assert lay["ls_iters"][0] == lay["niter_cost"][0] + lay["niter_cost"][1]      # next to niter_cost
    assert np.array_equal(counts, np.round(counts))
    assert (counts >= 0).all() and (counts.sum(1) <= ITER * LS_ITER).all()
