"""The root body in a body slot of its own (rr_kernel.h RR_ROOT_SLOT): the fixed-dimension instances of rodent_optimized run the tree
phases -- kinematics, com_pos, velocity sweep, backward sweep -- with the 64 bodies that are not the root in the first body slot (bodies
64 and 65 on lanes 0 and 1) and the root alone in the second, and that must not change a bit of anything the kernel writes.
`Batch.set_root_slot(False)` runs the same production single-step instance built with the plain map body = lane + 64 * slot
(rr_twoslot_kernel), so the two can be compared in one library.

The sample is tools/solver_trim_sample.py's: 48 states in contact after 30 env steps of seeded random actions and 16 reset states
(qacc_warmstart = 0).  One launch of the debug-dump instance per case shows that the states are in contact, i.e. that the tree phases'
results pass through a solver that runs."""
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
TREE_OUT = ("xpos", "xmat", "subtree_com", "cinert", "cvel", "qfrc_actuator")
MOVED = (1, 64, 65)      # the bodies whose lane slot differs between the two maps


@pytest.fixture(scope="module")
def sample():
    """The CPU-chosen states (float32 oracle) and the action of the step that follows, on the device."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import solver_trim_sample
    assert (solver_trim_sample.MODEL, solver_trim_sample.N) == (MODEL, N)
    _, st, ctrl = solver_trim_sample.sample()
    dev = torch.device("cuda:0")
    return {k: torch.tensor(st[k], dtype=torch.float32, device=dev) for k in STATE}, torch.tensor(ctrl, dtype=torch.float32, device=dev)


def _batch(cap, n=N):
    from rodent_amd import assets, hip
    return hip.Batch(hip.Model(assets.asset_path(MODEL), cap, LS_ITER, solver="cg"), n, torch.device("cuda:0"))


def _env_launch(cap, n_frames, st, ctrl, root_slot):
    """One env step of `n_frames` substeps through the production single-step instance: everything it writes, as int32 bit patterns."""
    from tests import util
    dev = torch.device("cuda:0")
    batch = _batch(cap)
    cost = torch.zeros(N, dtype=torch.int32, device=dev)
    batch.set_schedule(None, cost)
    batch.set_root_slot(root_slot)
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


def _tree_launch(cap, st, ctrl, root_slot):
    """One substep through pipeline_step with the tree phases' own outputs, as int32 bit patterns."""
    dev = torch.device("cuda:0")
    batch = _batch(cap)
    batch.set_root_slot(root_slot)
    d = batch.dims
    sizes = dict(xpos=3 * d.nbody, xmat=9 * d.nbody, subtree_com=3, cinert=10 * d.nbody, cvel=6 * d.nbody, qfrc_actuator=d.nv)
    out = {k: torch.zeros(N, sizes[k], device=dev) for k in TREE_OUT}
    s = {k: v.clone() for k, v in st.items()}
    batch.pipeline_step(s, ctrl, 1, out=out)
    torch.cuda.synchronize()
    res = {k: v.view(torch.int32).cpu().numpy() for k, v in out.items()}
    res.update({k: v.view(torch.int32).cpu().numpy() for k, v in s.items()})
    return res


def _debug_dump(cap, n_frames, st, ctrl):
    """The same substeps through the debug-dump instance: the dump of the last one, as numbers."""
    dev = torch.device("cuda:0")
    batch = _batch(cap)
    dbg = torch.zeros(N, batch.dims.dbg_floats, device=dev)
    batch.pipeline_step({k: v.clone() for k, v in st.items()}, ctrl, n_frames, out=dict(debug=dbg))
    torch.cuda.synchronize()
    num = dbg.cpu().numpy()
    return {name: num[:, o:o + n] for name, (o, n) in batch.debug_layout().items()}


@pytest.fixture(scope="module")
def launches(sample):
    """{(cap, substeps): (plain map, root slot, debug dump)}: every launch once, shared by the tests below."""
    st, ctrl = sample
    return {(cap, nf): (_env_launch(cap, nf, st, ctrl, False), _env_launch(cap, nf, st, ctrl, True), _debug_dump(cap, nf, st, ctrl))
            for cap in CAPS for nf in FRAMES}


@pytest.mark.parametrize("n_frames", FRAMES)
@pytest.mark.parametrize("cap", CAPS)
def test_root_slot_equals_plain_map(launches, cap, n_frames):
    """qpos, qvel, act, qacc_warmstart, obs, reward, done, metrics and the work estimate are bitwise equal, on states in contact."""
    off, on, dump = launches[(cap, n_frames)]
    n_act = (dump["con_dist"] < 0).sum(1)
    print("cap", cap, "substeps", n_frames, "| envs with a contact in penetration", int((n_act > 0).sum()))
    assert set(off) == set(on) == set(STATE) | {"obs", "reward", "done", "metrics", "work"}
    differing = [(k, int((off[k] != on[k]).sum())) for k in off if not np.array_equal(off[k], on[k])]
    print("differing", differing)
    assert not differing, differing
    assert np.isfinite(on["qpos"].view(np.float32)).all() and np.isfinite(on["obs"].view(np.float32)).all()
    assert (on["work"] > 0).any()
    # not vacuous: the states are in contact
    assert int((dump["kernarg_ok"] != 0).all())
    assert int((n_act > 0).sum()) >= 16


@pytest.mark.parametrize("cap", CAPS)
def test_tree_outputs_of_one_substep(sample, cap):
    """xpos, xmat, subtree_com, cinert, cvel and qfrc_actuator of one substep are bitwise equal, and the bodies that change slot move."""
    st, ctrl = sample
    off, on = _tree_launch(cap, st, ctrl, False), _tree_launch(cap, st, ctrl, True)
    assert set(off) == set(on) == set(TREE_OUT) | set(STATE)
    differing = [(k, int((off[k] != on[k]).sum())) for k in off if not np.array_equal(off[k], on[k])]
    print("cap", cap, "differing", differing)
    assert not differing, differing
    for k in TREE_OUT:
        assert np.isfinite(on[k].view(np.float32)).all(), k
    # the 48 contact states (the sample's first rows) carry velocity: the rows of the moved bodies are exercised, not zeros
    cvel = on["cvel"].view(np.float32).reshape(N, -1, 6)
    cinert = on["cinert"].view(np.float32).reshape(N, -1, 10)
    for b in MOVED:
        assert (np.abs(cvel[:48, b]).max(1) > 0).all(), b
        assert (np.abs(cinert[:48, b]).max(1) > 0).all(), b


def test_switch_refusals():
    """The switch is refused, in words, for another model, and a batch with the switch off refuses the launches it has no instance for."""
    from rodent_amd import assets, hip
    dev = torch.device("cuda:0")
    other = hip.Batch(hip.Model(assets.asset_path("rodent_new"), 8, LS_ITER, solver="cg"), 4, dev)
    with pytest.raises(RuntimeError, match="rr_batch_set_root_slot: only the fixed-dimension CG instance of the rodent_optimized model"):
        other.set_root_slot(False)
    other.set_root_slot(True)
    batch = _batch(8, 4)
    batch.set_root_slot(False)
    d = batch.dims
    dbg = torch.zeros(4, d.dbg_floats, device=dev)
    with pytest.raises(RuntimeError, match="rr_batch_set_root_slot\\(b, 0\\) serves production launches only"):
        batch.pipeline_step(batch.zeros_state(), torch.zeros(4, d.nu, device=dev), 1, out=dict(debug=dbg))
    # a multi-step launch: refused before anything is launched
    from tests import util
    env = dict(track_pos=torch.tensor(util.synthetic_track(), dtype=torch.float32, device=dev), cur_frame=torch.zeros(4, dtype=torch.int32, device=dev),
               obs=torch.zeros(4, d.obs_dim, device=dev), reward=torch.zeros(4, device=dev), done=torch.zeros(4, device=dev),
               metrics=torch.zeros(4, 3, device=dev))
    wrap = dict(first=batch.zeros_state(), first_obs=torch.zeros(4, d.obs_dim, device=dev), prev_done=torch.zeros(4, device=dev),
                steps_in=torch.zeros(4, device=dev), steps_out=torch.zeros(4, device=dev), truncation_out=torch.zeros(4, device=dev), episode_length=1000)
    with pytest.raises(RuntimeError, match="rr_batch_set_root_slot\\(b, 0\\): the instance with the plain lane-to-body map is single-step"):
        batch.env_unroll(batch.zeros_state(), batch.zeros_state(), torch.zeros(2, 4, d.nu, device=dev), 1, env,
                         torch.zeros(4, dtype=torch.int32, device=dev), wrap)
    torch.cuda.synchronize()
