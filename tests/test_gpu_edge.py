"""GPU edge cases of the HIP path against the oracle: no contact / every contact active / many limits active,
clamped and saturating inputs, odd batch sizes, n_frames variants, argument errors."""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _batch(N, model="rodent_optimized", it=(8, 8)):
    from rodent_amd import assets, hip
    return hip.Batch(hip.Model(assets.asset_path(model), *it), N, torch.device(DEV))


def _run_substep(ref, M, qpos, qvel, act, warm, ctrl):
    d = ref.RefData(M)
    d.set("qpos", qpos); d.set("qvel", qvel); d.set("act", act); d.set("qacc_warmstart", warm)
    d.step(ctrl, 1)
    return d


@pytest.mark.parametrize("scenario", ["airborne", "pressed_into_floor", "limits_violated"])
def test_contact_and_limit_extremes(scenario, oracle_built):
    from rodent_amd import assets, mjcf
    ref = oracle_built
    path = assets.asset_path("rodent_optimized")
    m = mjcf.load_blob(path)
    M = ref.RefModel(path, "f64"); M.set_iterations(8, 8)
    N = 5                                            # odd batch size on purpose
    rng = np.random.default_rng(3)
    q = np.tile(m["qpos0"].astype(np.float64), (N, 1))
    if scenario == "airborne":
        q[:, 2] = 1.0                                # no contact, solver sees only (possibly) limit rows
    elif scenario == "pressed_into_floor":
        q[:, 2] = 0.012                              # belly on the floor: (almost) every contact active
        q[:, 7:] += rng.uniform(-0.02, 0.02, (N, M.nq - 7))
    else:
        q[:, 7:] += rng.uniform(-1.5, 1.5, (N, M.nq - 7))   # far outside most joint ranges
        q[:, 2] = 0.5
    v = rng.uniform(-0.5, 0.5, (N, M.nv))
    act = rng.uniform(-1, 1, (N, M.nu)); warm = np.zeros((N, M.nv))
    ctrl = rng.uniform(-3, 3, (N, M.nu))             # outside ctrlrange: clamped to [-1, 1] by the actuator model
    b = _batch(N)
    st = {k: torch.tensor(x, dtype=torch.float32, device=DEV) for k, x in dict(qpos=q, qvel=v, act=act, qacc_warmstart=warm).items()}
    dbg = torch.zeros(N, b.dims.dbg_floats, device=DEV)
    b.pipeline_step(st, torch.tensor(ctrl, dtype=torch.float32, device=DEV), 1, out=dict(debug=dbg))
    torch.cuda.synchronize()
    lay = b.debug_layout()
    dbg = dbg.cpu().numpy().astype(np.float64)
    nact, nlim = [], []
    for e in range(N):
        d = _run_substep(ref, M, q[e], v[e], act[e], warm[e], ctrl[e])
        active = d.get("con_dist") < 0
        nact.append(int(active.sum())); nlim.append(int((d.get("efc_pos")[:M.nlimit] < 0).sum()))
        o, n = lay["con_dist"]
        assert np.array_equal(dbg[e, o:o + n] < 0, active)                       # same active set (integer-exact)
        for name, tol in (("qacc_smooth", 5e-3), ("qfrc_actuator", 1e-5), ("qM", 1e-4)):
            o, n = lay[name]
            want = d.get(name)
            assert np.abs(dbg[e, o:o + n] - want).max() <= tol * max(np.abs(want).max(), 1e-6), (scenario, name)
        qv = d.get("qvel")
        dv = np.abs(qv - v[e]).max()
        assert np.abs(st["qvel"][e].cpu().numpy() - qv).max() <= 5e-3 * max(dv, 1e-2), scenario
        assert np.abs(st["act"][e].cpu().numpy() - d.get("act")).max() < 1e-6
    if scenario == "airborne":
        assert max(nact) == 0
    if scenario == "pressed_into_floor":
        assert min(nact) >= 30
    if scenario == "limits_violated":
        assert min(nlim) >= 20
    assert torch.isfinite(st["qpos"]).all() and torch.isfinite(st["qvel"]).all()


def test_cur_frame_saturates_like_a_clamped_gather(oracle_built):
    """info['cur_frame'] is never reset by AutoReset, so it runs past the clip: JAX clamps the gather index."""
    from rodent_amd import envs
    track = util.synthetic_track(T=20)
    env = envs.get_environment("rodent", track_pos=track, num_envs=3, xml_path="rodent_optimized.xml", iterations=8,
                               ls_iterations=8, device=DEV, pipeline_outputs=True)
    s = env.reset(1)
    s.info["cur_frame"] = torch.tensor([18, 19, 400], dtype=torch.int32, device=DEV)
    n = env.step(s, torch.zeros(3, env.action_size, device=DEV))
    assert n.info["cur_frame"].tolist() == [19, 20, 401]
    xq = n.pipeline_state
    # local tracking vector uses track_pos[min(frame + 1, T - 1)] = the last row for all three envs
    want = torch.tensor(track[-1], dtype=torch.float32, device=DEV) - xq.qpos[:, :3]
    xm1 = xq.xmat[:, 1].reshape(3, 3, 3)
    torch.testing.assert_close(n.obs[:, -3:], torch.einsum("nij,nj->ni", xm1, want), rtol=1e-5, atol=1e-6)
    assert torch.isfinite(n.reward).all()


@pytest.mark.parametrize("n_frames", [1, 3, 10])
def test_n_frames_and_single_env(n_frames, oracle_built):
    from rodent_amd import assets, mjcf
    ref = oracle_built
    path = assets.asset_path("rodent_new")
    m = mjcf.load_blob(path)
    M = ref.RefModel(path, "f64"); M.set_iterations(6, 6)        # the env class' default solver setting
    q = m["qpos0"].astype(np.float64); q[2] = 0.05
    b = _batch(1, "rodent_new", (6, 6))
    st = dict(qpos=torch.tensor(q[None], dtype=torch.float32, device=DEV), qvel=torch.zeros(1, M.nv, device=DEV),
              act=torch.zeros(1, M.nu, device=DEV), qacc_warmstart=torch.zeros(1, M.nv, device=DEV))
    ctrl = np.linspace(-1, 1, M.nu)
    b.pipeline_step(st, torch.tensor(ctrl[None], dtype=torch.float32, device=DEV), n_frames)
    d = ref.RefData(M)
    d.set("qpos", q)
    d.step(ctrl, n_frames)
    assert np.abs(st["qpos"][0].cpu().numpy() - d.get("qpos")).max() < 1e-4


def test_argument_errors_are_reported_not_crashed():
    b = _batch(4)
    st = b.zeros_state()
    with pytest.raises(ValueError):
        b.pipeline_step(st, torch.zeros(3, b.dims.nu, device=DEV), 1)             # wrong batch size
    with pytest.raises(ValueError):
        b.pipeline_step(st, torch.zeros(4, b.dims.nu), 1)                          # host tensor
    with pytest.raises(RuntimeError, match="n_frames"):
        b.pipeline_step(st, torch.zeros(4, b.dims.nu, device=DEV), 0)
    bad = dict(st); bad["qpos"] = st["qpos"].double()
    with pytest.raises(ValueError):
        b.pipeline_init(bad)


def test_optional_outputs_all_null_and_all_set(oracle_built):
    """The debug-dump instance with every optional rr_outputs pointer NULL except the dump, and with all of them set: the
    kernel's re-read of its I/O block through the kernarg segment must equal the real parameter (dump field `kernarg_ok`),
    the states must be bit-identical, and the contact geometry outputs / pose outputs must equal the dump's fields."""
    from rodent_amd import assets
    ref = oracle_built
    N = 8
    b = _batch(N)
    st, M, m = util.settled_states(ref, "rodent_optimized", N, seed=8, iterations=(8, 8))
    ctrl = torch.tensor(np.random.default_rng(1).uniform(-1, 1, (N, M.nu)), dtype=torch.float32, device=DEV)
    mk = lambda: {k: torch.tensor(v, dtype=torch.float32, device=DEV).contiguous() for k, v in st.items()}
    d = b.dims
    dbg1 = torch.zeros(N, d.dbg_floats, device=DEV)
    s1 = mk()
    b.pipeline_step(s1, ctrl, 1, out=dict(debug=dbg1))
    full = dict(cinert=torch.zeros(N, d.nbody * 10, device=DEV), cvel=torch.zeros(N, d.nbody * 6, device=DEV),
                qfrc_actuator=torch.zeros(N, d.nv, device=DEV), xpos=torch.zeros(N, d.nbody * 3, device=DEV),
                xmat=torch.zeros(N, d.nbody * 9, device=DEV), subtree_com=torch.zeros(N, 3, device=DEV),
                debug=torch.zeros(N, d.dbg_floats, device=DEV), contact_dist=torch.zeros(N, d.ncon, device=DEV),
                contact_pos=torch.zeros(N, d.ncon * 3, device=DEV), contact_frame=torch.zeros(N, d.ncon * 9, device=DEV))
    s2 = mk()
    b.pipeline_step(s2, ctrl, 1, out=full)
    s3 = mk()
    b.pipeline_step(s3, ctrl, 1, out=dict(contact_dist=torch.zeros(N, d.ncon, device=DEV)))      # debug instance, no dump buffer
    s4 = mk()
    b.pipeline_step(s4, ctrl, 1)                                                                   # production instance, out = NULL
    torch.cuda.synchronize()
    lay = b.debug_layout()
    o, n = lay["kernarg_ok"]
    assert (dbg1[:, o] == 1).all() and (full["debug"][:, o] == 1).all()
    for k in s1:
        assert torch.equal(s1[k], s2[k]) and torch.equal(s1[k], s3[k]), k
        assert torch.isfinite(s4[k]).all()
    f = lambda name: full["debug"][:, lay[name][0]:lay[name][0] + lay[name][1]]
    assert torch.equal(full["contact_dist"], f("con_dist")) and torch.equal(full["contact_pos"], f("con_pos"))
    assert torch.equal(full["contact_frame"], f("con_frame"))
    assert torch.equal(full["xpos"], f("xpos")) and torch.equal(full["xmat"], f("xmat")) and torch.equal(full["cinert"], f("cinert"))
    assert torch.equal(full["cvel"], f("cvel")) and torch.equal(full["qfrc_actuator"], f("qfrc_actuator"))
    # contact geometry against the oracle (brax State.contact: dist, pos, frame)
    for e in range(N):
        dd = util.oracle_forward(ref, M, st, e, ctrl[e].cpu().numpy().astype(np.float64))
        assert np.abs(full["contact_dist"][e].cpu().numpy() - dd.get("con_dist")).max() < 2e-6
        assert np.abs(full["contact_pos"][e].cpu().numpy() - dd.get("con_pos")).max() < 2e-6
        assert np.abs(full["contact_frame"][e].cpu().numpy() - dd.get("con_frame")).max() < 2e-6


def test_env_contact_and_pipeline_outputs():
    """`Rodent(..., pipeline_outputs=True, contact_outputs=True)`: brax-style State.contact fields and `sys` id tables."""
    from rodent_amd import envs
    env = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=4, xml_path="rodent_optimized.xml", iterations=8,
                               ls_iterations=8, device=DEV, pipeline_outputs=True, contact_outputs=True)
    r = env.reset(2)
    s = env.step(r, torch.zeros(4, env.action_size, device=DEV))
    ps = s.pipeline_state
    assert ps.contact_dist.shape == (4, 59) and ps.contact_pos.shape == (4, 59, 3) and ps.contact_frame.shape == (4, 59, 3, 3)
    assert torch.isfinite(ps.contact_dist).all() and ps.xpos.shape == (4, 66, 3)
    assert torch.allclose(ps.contact_frame[:, :, 0], torch.tensor([0.0, 0.0, 1.0], device=DEV).expand(4, 59, 3))     # floor normal
    assert env.sys.contact_geom2[-5:].tolist() == [1, 62, 75, 89, 97] and env.sys.contact_link_idx[0].tolist() == [-1] * 59
    c = env.contact(ps)                                   # brax State.contact, fields as in [NB mjcf.ipynb:917-921]
    assert c.geom2.dtype == torch.int32 and c.geom2[-5:].tolist() == [1, 62, 75, 89, 97] and c.geom1.tolist() == [0] * 59
    assert c.link_idx[1].tolist() == (env.sys.geom_bodyid[env.sys.contact_geom2] - 1).tolist()
    assert c.friction.shape == (59, 5) and torch.allclose(c.friction[0], torch.tensor([1.5, 1.5, 0.005, 1e-4, 1e-4], device=DEV))
    assert torch.allclose(c.solimp[0], torch.tensor([0.9, 0.95, 0.001, 0.5, 2.0], device=DEV)) and float(c.elasticity.abs().max()) == 0
    assert c.dist is ps.contact_dist
    lean = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=4, xml_path="rodent_optimized.xml", iterations=8,
                                ls_iterations=8, device=DEV)
    r2 = lean.reset(2)
    s2 = lean.step(r2, torch.zeros(4, env.action_size, device=DEV))
    assert s2.pipeline_state.cinert is None and s2.pipeline_state.contact_dist is None and torch.isfinite(s2.obs).all()
    # contact outputs are served by the debug-dump instance, the lean env by the production one: equal to rounding, which one
    # forward pass (reset) shows; ten substeps amplify it (tests/parity.py)
    assert torch.equal(r2.pipeline_state.qpos, r.pipeline_state.qpos) and torch.allclose(r2.obs, r.obs, atol=1e-5, rtol=1e-5)


# Which launch forms each shipped blob serves (the table of DESIGN.md section 4h): None = served, a string = the fragment of the
# refusal's message, SKIP = a cell another test pins -- the evaluation refusals of Newton on rodent_optimized and of rodent_pair in
# test_gpu_eval_unroll.py::test_refusals, the per-env parameter refusals of rodent_cpu, rodent_pair and Newton on rodent_optimized in
# test_gpu_randomisation.py::test_refusals, the multi-step refusal of Newton on rodent_optimized in test_gpu_env.py.
SKIP = "(pinned elsewhere)"
NO_DIAG = "no diagnostic kernel instance"
_ALL = dict(debug=None, profile=None, unroll=None, eval=None, params=None)
_NEWTON = dict(debug=None, profile=NO_DIAG, unroll="multi-step", eval="Newton", params="Newton")
LAUNCH_FORMS = {
    ("rodent_0", "cg"): _ALL,                     # (2,2,1) slot counts, generic dimensions
    ("rodent_new", "cg"): _ALL,                   # fixed-dimension instances
    ("rodent_optimized", "cg"): _ALL,
    ("rodent_cpu", "cg"): dict(debug=None, profile=NO_DIAG, unroll=None, eval=None, params=SKIP),             # candidate-pair contacts
    ("rodent_pair", "cg"): dict(debug=None, profile=NO_DIAG, unroll="multi-step", eval=SKIP, params=SKIP),    # (3,3,2) + the two-wave pair instance
    ("rodent_0", "newton"): _NEWTON,
    ("rodent_new", "newton"): _NEWTON,
    ("rodent_optimized", "newton"): dict(_NEWTON, unroll=SKIP, eval=SKIP, params=SKIP),
}


@pytest.mark.parametrize("model,solver", list(LAUNCH_FORMS), ids=["-".join(k) for k in LAUNCH_FORMS])
def test_launch_forms_of_the_shipped_models(model, solver):
    """Every launch form a shipped blob serves runs once and leaves a finite state; every form it does not serve is refused with
    the reason (4 envs, n_frames = 1, 2 steps per multi-step launch, 2 solver iterations)."""
    from rodent_amd import assets, envs, hip, jax_random
    from rodent_amd.envs import wrappers
    from rodent_amd.training import acting, networks
    from tests import randomisation_sets as rs
    want = LAUNCH_FORMS[(model, solver)]
    n, T = 4, 2
    if model in ("rodent_cpu", "rodent_pair"):
        with pytest.raises(RuntimeError, match="Newton instance"):
            hip.Model(assets.asset_path(model), 2, 2, solver="newton")
    env = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=n, xml_path=model + ".xml", solver=solver, iterations=2,
                               ls_iterations=2, n_frames=1, device=DEV, healthy_z_range=(-0.3, 0.5))
    b, nu = env._batch, env.action_size
    finite = lambda s: all(bool(torch.isfinite(getattr(s.pipeline_state, k)).all()) for k in ("qpos", "qvel", "act", "qacc_warmstart"))

    def attempt(form, fn):
        """fn() launches and returns the state(s) it left; the table says whether it runs or which refusal it meets."""
        if want[form] is None:
            assert all(finite(s) for s in fn()), form
        elif want[form] is not SKIP:
            with pytest.raises(RuntimeError, match=want[form]):
                fn()

    def physics(out=None):
        st = b.zeros_state()
        st["qpos"][:] = torch.from_numpy(env.sys.qpos0).to(DEV)
        b.pipeline_step(st, torch.zeros(n, nu, device=DEV), 1, out=out)
        return [envs.State(envs.PipelineState(**st), None, None, None)]

    def profiled():
        b.set_profile(torch.zeros(n, 16, dtype=torch.int64, device=DEV))
        try:
            return physics()
        finally:
            b.set_profile(None)

    keys = jax_random.split(jax_random.PRNGKey(5), n)
    torch.manual_seed(5)
    actor = acting.actor_params(networks.make_ppo_networks(env.observation_size, nu, device=DEV).policy_network, None, 0.001)
    wenv = wrappers.wrap(env, episode_length=5, action_repeat=1)
    assert isinstance(wenv, wrappers.FusedEpisodeAutoResetWrapper)

    def unrolled(with_actor):
        if not with_actor:
            return [wenv.unroll(wenv.reset(keys), torch.zeros(T, n, nu, device=DEV))]
        K = env.observation_size
        traj = dict(obs=torch.empty(n, T + 1, K, device=DEV), raw_action=torch.empty(n, T, nu, device=DEV),
                    **{k: torch.empty(n, T, device=DEV) for k in ("log_prob", "reward", "discount", "truncation")})
        return [wenv.unroll_policy(wenv.reset(keys), actor, torch.randn(T, n, nu, device=DEV), traj)[0]]

    assert finite(env.step(env.reset(keys), torch.zeros(n, nu, device=DEV)))                 # single step, production instance
    assert all(finite(s) for s in physics())                                                   # physics only (rodent_pair: the two-wave instance)
    attempt("debug", lambda: physics(dict(debug=torch.zeros(n, b.dims.dbg_floats, device=DEV))))
    attempt("profile", profiled)
    served = want["unroll"] is None
    assert b.unroll_supported(False) == served and b.unroll_supported(True) == served
    attempt("unroll", lambda: unrolled(False))
    attempt("unroll", lambda: unrolled(True))
    assert env.eval_supported() == (want["eval"] is None)
    attempt("eval", lambda: [env.unroll_eval(env.reset(keys), T, actor)])
    assert b.env_params_supported() == (want["params"] is None)
    fn = rs.system_fn(rs.mixed_fields)

    def randomised():
        env.randomize(lambda sys: fn(sys, n))
        return [env.step(env.reset(keys), torch.zeros(n, nu, device=DEV))]
    attempt("params", randomised)
    torch.cuda.synchronize()
