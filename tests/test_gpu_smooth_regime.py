"""Per-entry parity of the step kernel in the smooth regime (tests/smooth_regime.py; DESIGN.md section 2, "Per-entry parity"): every
kernel instance on the free variant of its model, 64 airborne envs at |qvel| <= 5 with the joints over their whole range, held to the
float64 oracle ENTRY BY ENTRY -- each entry's largest error over the samples divided by that entry's own largest magnitude, the maximum
taken over all samples and entries -- within 3x the worse of the oracle's two float32 builds on the same inputs + 2^-22.  The regime
facts (0 solver iterations, nothing within 1e-4 of contact, no limit row) are asserted on the float64 oracle before anything is
compared; tests/test_smooth_regime_cpu.py holds the criterion itself (accepts a float32 evaluation, rejects a 5 % error in one distal
parameter 10x over).  Each case records its figures with the ladder's `_report`, as ladder_smooth_<case>.json."""
import numpy as np
import pytest
import torch

from rodent_amd import mjcf
from tests import randomisation_sets as rs, smooth_regime as sr, util
from tests.hip_impl import HipImpl
from tests.test_gpu_ladder import _report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = sr.N


@pytest.fixture(autouse=True)
def _oracle(oracle_built):
    return oracle_built


def _judge(name, fields, got, want, yards, tab, extra=None):
    """Record R of the kernel and of both float32 oracles per field, then assert the criterion."""
    rec, bad = sr.judge(fields, got, want, yards, tab)
    _report("smooth_" + name, dict(extra or {}, fields=rec))
    assert not bad, (name, {f: dict(rec[f], worst_entry_sample_error=sr.worst_entries(f, got[f], want[f], tab)) for f in bad})


def _dev(a, dtype=torch.float32):
    return torch.tensor(a, dtype=dtype, device=DEV).contiguous()


def _oracles(make, *inputs):
    """(float64 result with the regime facts asserted, [f32 result, f32fma result]); `make(precision)` -> an oracle driver."""
    want = make("f64").regime_facts(*inputs)
    run = lambda o: (o.steps if hasattr(o, "steps") else o.step)(*inputs)
    return want, [run(make(p)) for p in ("f32", "f32fma")]


def _hip_step(batch, st, ctrl, n_frames, dbg=None):
    ds = {k: _dev(st[k]) for k in sr.STATE}
    batch.pipeline_step(ds, _dev(ctrl), n_frames, out=dict(debug=dbg) if dbg is not None else None)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy().astype(np.float64) for k, v in ds.items()}
    out["qacc"] = out["qacc_warmstart"]                      # the warm start handed on IS the solver's qacc
    return out


def test_debug_dump_instance(tmp_path):
    """rodent_optimized, one substep through the instance that dumps its stages: the smooth dynamics field by field, the solver's
    result and the stepped state."""
    stem = sr.free_blob("rodent_optimized", tmp_path)
    tab = mjcf.load_blob(stem + ".rrm")
    st, ctrl, _ = sr.smooth_states("rodent_optimized", seed=0)
    want, yards = _oracles(lambda p: sr.Oracle(stem, N, p), st, ctrl, 1)
    impl = HipImpl(stem, N, (8, 8), True)
    got = _hip_step(impl.batch, st, ctrl, 1, impl.dbg)
    g = impl.dbg.cpu().numpy().astype(np.float64)
    f = lambda name: g[:, impl.lay[name][0]:impl.lay[name][0] + impl.lay[name][1]]
    np.testing.assert_array_equal(f("qacc").astype(np.float32), got["qacc"].astype(np.float32))
    for k in sr.STAGE_FIELDS[:-1]:
        got[k] = f(k)
    niter, dist = f("niter_cost")[:, 0], f("con_dist")
    print("debug dump: niter max", niter.max(), "smallest con_dist", dist.min(), "float32 oracles' iterations", [int(y["niter_sum"].max()) for y in yards])
    assert (dist >= 0).all()
    _judge("debug_dump", sr.STAGE_FIELDS + sr.STEP_FIELDS[1:], got, want, yards, tab, dict(niter_max=niter.max(), min_con_dist=dist.min()))
    assert (niter == 0).all(), niter


PRODUCTION = {      # case -> (model, seed, fixed_instance or None, solver, iterations)
    "rodent_optimized": ("rodent_optimized", 0, 1, None, (8, 8)), "rodent_new": ("rodent_new", 0, 1, None, (8, 8)),
    "rodent_0": ("rodent_0", 0, 0, None, (8, 8)), "rodent_cpu": ("rodent_cpu", 0, None, None, (8, 8)),
    "rodent_pair": ("rodent_pair", 0, None, None, (8, 8)), "newton": ("rodent_optimized", 3, None, "newton", (4, 8)),
}


@pytest.mark.parametrize("case", list(PRODUCTION))
def test_production_instance_one_substep(tmp_path, case):
    """The instances without a dump, one substep each: the fixed-dimension instances (the edited blob must still select them), the
    generic (2,2,1) one, the candidate-pair one (nothing dropped), the two-wave one (both replicas airborne), the Newton solver."""
    from rodent_amd import hip
    model, seed, fixed, solver, it = PRODUCTION[case]
    stem = sr.free_blob(model, tmp_path)
    tab = mjcf.load_blob(stem + ".rrm")
    if fixed is not None:
        assert hip.Model(stem + ".rrm").dims.fixed_instance == fixed
    st, ctrl, draws = sr.smooth_states(model, seed=seed)
    want, yards = _oracles(lambda p: sr.Oracle(stem, N, p, it, solver or "cg"), st, ctrl, 1)
    impl = HipImpl(stem, N, it, False, solver=solver)
    got = _hip_step(impl.batch, st, ctrl, 1)
    assert impl.batch.contact_overflow() == 0
    _judge("production_" + case, sr.STEP_FIELDS, got, want, yards, tab, dict(draws=draws, min_con_dist=want["min_con_dist"]))


def test_per_env_parameter_batch_one_substep(tmp_path):
    """Env e on parameter set e % 3 of tests/randomisation_sets.py (the rr_rand_kernel instance), each env against the oracle on ITS set's
    blob, all written from the free variant."""
    from rodent_amd import envs
    stem = sr.free_blob("rodent_optimized", tmp_path)
    tab = mjcf.load_blob(stem + ".rrm")
    stems = rs.write_blobs(stem, tmp_path)
    st, ctrl, _ = sr.smooth_states("rodent_optimized", seed=3)
    want, yards = _oracles(lambda p: sr.GroupedOracle(stems, N, p), st, ctrl, 1)
    env = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=N, xml_path=stem + ".rrm", iterations=8, ls_iterations=8, device=DEV)
    fn = rs.system_fn(rs.mixed_fields)
    env.randomize(lambda sys: fn(sys, N))
    assert env.env_params() is not None
    got = _hip_step(env._batch, st, ctrl, 1)
    _judge("production_parameter_sets", sr.STEP_FIELDS, got, want, yards, tab)
    # the sets do differ at this resolution: the shipped parameters on every env are far outside
    plain = _hip_step(HipImpl(stem, N, (8, 8), False).batch, st, ctrl, 1)
    assert sr.judge(("qacc",), plain, want, yards, tab)[1] == ["qacc"]


@pytest.mark.parametrize("model", sr.FLOOR_MODELS)
def test_ten_substeps_in_one_launch(tmp_path, model):
    """n_frames = 10: the facts hold after the tenth substep, the state after it per entry."""
    stem = sr.free_blob(model, tmp_path)
    tab = mjcf.load_blob(stem + ".rrm")
    st, ctrl, _ = sr.smooth_states(model, seed=0)
    want, yards = _oracles(lambda p: sr.Oracle(stem, N, p), st, ctrl, 10)
    got = _hip_step(HipImpl(stem, N, (8, 8), False).batch, st, ctrl, 10)
    _judge("ten_substeps_" + model, sr.STEP_FIELDS, got, want, yards, tab, dict(min_con_dist=want["min_con_dist"]))


# ------------------------------------------------------------------------------------------ env forms
def _env(stem, **kw):
    from rodent_amd import envs
    return envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=N, xml_path=stem + ".rrm", iterations=8, ls_iterations=8,
                                device=DEV, **kw)


def _start(env, st, cur_frame):
    """A reset state of `env` (wrapped or not) with the pipeline state and the frame counters replaced."""
    s0 = env.reset(0)
    info = dict(s0.info)
    info["cur_frame"] = _dev(cur_frame, torch.int32)
    return s0.replace(pipeline_state=s0.pipeline_state.replace(**{k: _dev(st[k]) for k in sr.STATE}), info=info)


def _env_result(s, tab):
    torch.cuda.synchronize()
    out = dict(qpos=s.pipeline_state.qpos.cpu().numpy().astype(np.float64), qvel=s.pipeline_state.qvel.cpu().numpy().astype(np.float64),
               obs=s.obs.cpu().numpy().astype(np.float64))
    assert np.array_equal(out["obs"][:, :out["qpos"].shape[1]].astype(np.float32), out["qpos"].astype(np.float32))       # the obs carries the state itself
    return sr.obs_fields(out, tab)


def _env_case(tmp_path, steps, vz, seed):
    stem = sr.free_blob("rodent_optimized", tmp_path)
    tab = mjcf.load_blob(stem + ".rrm")
    st, actions, cur_frame = sr.env_inputs("rodent_optimized", steps, vz, seed)
    want, yards = _oracles(lambda p: sr.OracleEnv(stem, N, p, util.synthetic_track()), st, actions, cur_frame)
    return stem, tab, st, actions, cur_frame, want, [sr.obs_fields(y, tab) for y in yards]


def test_env_steps(tmp_path):
    """Three env steps (30 substeps) through `Rodent.step`."""
    stem, tab, st, actions, cur_frame, want, yards = _env_case(tmp_path, *sr.ENV_CASES[0])
    env = _env(stem)
    s = _start(env, st, cur_frame)
    for a in actions:
        s = env.step(s, _dev(a))
        assert (s.done == 0).all()
    assert np.array_equal(s.info["cur_frame"].cpu().numpy(), want["cur_frame"])
    _judge("env_steps", sr.OBS_FIELDS, _env_result(s, tab), sr.obs_fields(want, tab), yards, tab)


def test_env_unroll(tmp_path):
    """The same three steps as ONE launch of the multi-step instance under Episode(1000) + AutoReset: no episode ends, nothing is restored."""
    from rodent_amd.envs import wrappers
    stem, tab, st, actions, cur_frame, want, yards = _env_case(tmp_path, *sr.ENV_CASES[0])
    wenv = wrappers.wrap(_env(stem), episode_length=1000, action_repeat=1)
    s0 = _start(wenv, st, cur_frame)
    s = wenv.unroll(s0, _dev(actions))
    torch.cuda.synchronize()
    assert (s.done == 0).all() and (s.info["steps"] == len(actions)).all() and (s.info["truncation"] == 0).all()
    assert not torch.equal(s.pipeline_state.qpos, s.info["first_pipeline_state"].qpos)
    assert np.array_equal(s.info["cur_frame"].cpu().numpy(), want["cur_frame"])
    _judge("env_unroll", sr.OBS_FIELDS, _env_result(s, tab), sr.obs_fields(want, tab), yards, tab)


def test_pose_env_step(tmp_path):
    """One env step of a pose-tracking env (rr_pose_kernel), at the full speeds: state and observation are those of the plain map."""
    stem, tab, st, actions, cur_frame, want, yards = _env_case(tmp_path, *sr.ENV_CASES[1])
    T = len(util.synthetic_track())
    quat = np.tile([1.0, 0.0, 0.0, 0.0], (T, 1))
    joints = np.tile(tab["qpos0"][7:].astype(np.float64), (T, 1))
    env = _env(stem, track_quat=quat, track_joints=joints)
    assert env.pose_tracking
    s = env.step(_start(env, st, cur_frame), _dev(actions[0]))
    assert (s.done == 0).all() and torch.isfinite(s.reward).all() and (s.metrics["joint_reward"] >= 0).all()
    assert np.array_equal(s.info["cur_frame"].cpu().numpy(), want["cur_frame"])
    _judge("pose_env_step", sr.OBS_FIELDS, _env_result(s, tab), sr.obs_fields(want, tab), yards, tab)
