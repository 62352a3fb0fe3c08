"""GPU parity: the HIP step kernel (through the C ABI) against the CPU oracle on the same seeded inputs.

Tolerances are float32 round-off scaled: the oracle runs in float64; per-stage fields of ONE forward
pass from identical inputs must agree to ~1e-4 of the field's scale (1e-5 for the pure-kinematics
fields); integer indices are bit-exact (tests/test_known_answers.py pins the contact id list).
"""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu


def _to_dev(st, dev):
    return {k: torch.tensor(v, dtype=torch.float32, device=dev).contiguous() for k, v in st.items()}


def _rel(a, b):
    scale = max(np.abs(b).max(), 1e-30)
    return np.abs(a - b).max() / scale


# field -> (oracle name, tolerance relative to the field's max magnitude)
# bounds are <= 10x the worst value measured on MI355X over the three models (gpurun_out/t_j.log of round 1, in brackets)
STAGES = [("xpos", "xpos", 3e-6), ("xquat", "xquat", 1e-6), ("xmat", "xmat", 2e-6),        # [6.5e-7, 1.7e-7, 3.5e-7]
          ("cinert", "cinert", 1e-7), ("crb", "crb", 1e-6), ("cdof", "cdof", 2e-6),        # [1.4e-8, 1.5e-7, 3.3e-7]
          ("cvel", "cvel", 3e-6), ("qM", "qM", 1e-6), ("qLD", "qLD", 6e-5),                # [5.0e-7, 1.5e-7, 1.1e-5]
          ("qfrc_bias", "qfrc_bias", 3e-6), ("qfrc_passive", "qfrc_passive", 6e-7),        # [4.3e-7, 9.8e-8]
          ("qfrc_actuator", "qfrc_actuator", 3e-6), ("qfrc_smooth", "qfrc_smooth", 3e-6),  # [4.3e-7, 4.3e-7]
          ("qacc_smooth", "qacc_smooth", 2e-5), ("con_dist", "con_dist", 5e-6),            # [3.6e-6, 7.7e-7]
          ("con_pos", "con_pos", 3e-6), ("con_frame", "con_frame", 2e-6)]                  # [4.5e-7, 3.0e-7]


@pytest.mark.parametrize("model_name", ["rodent_optimized", "rodent_new", "rodent_pair"])
def test_forward_stages_match_oracle(model_name, oracle_built):
    from rodent_amd import assets, hip
    ref = oracle_built
    N = 48 if model_name != "rodent_pair" else 16
    st, M, m = util.settled_states(ref, model_name, N, seed=1, iterations=(8, 8))
    dev = torch.device("cuda:0")
    model = hip.Model(assets.asset_path(model_name), iterations=8, ls_iterations=8)
    batch = hip.Batch(model, N, dev)
    rng = np.random.default_rng(5)
    ctrl = rng.uniform(-1, 1, (N, M.nu))
    ds = _to_dev(st, dev)
    dbg = torch.zeros(N, batch.dims.dbg_floats, device=dev)
    batch.pipeline_step(ds, torch.tensor(ctrl, dtype=torch.float32, device=dev), 1, out=dict(debug=dbg))
    torch.cuda.synchronize()
    lay = batch.debug_layout()
    dbg = dbg.cpu().numpy().astype(np.float64)
    worst = {}
    nact = nlim = 0
    lim_dof = m["jnt_dofadr"][m["limit_jnt"]]
    for e in range(N):
        d = util.oracle_forward(ref, M, st, e, ctrl[e])
        # limit rows (one per limited hinge): activity exact away from the switching point, D / aref of the active rows
        o, n = lay["limit_pos_D_aref"]
        lim = dbg[e, o:o + n].reshape(-1, 3)[lim_dof]
        lpos = d.get("efc_pos")[:M.nlimit]
        assert np.array_equal((lim[:, 0] < 0)[np.abs(lpos) > 2e-6], (lpos < 0)[np.abs(lpos) > 2e-6])
        la = lpos < -2e-6
        if la.any():
            nlim += int(la.sum())
            worst["lim_D"] = max(worst.get("lim_D", 0), _rel(lim[la, 1], d.get("efc_D")[:M.nlimit][la]))
            worst["lim_aref"] = max(worst.get("lim_aref", 0), _rel(lim[la, 2], d.get("efc_aref")[:M.nlimit][la]))
        for name, oname, tol in STAGES:
            o, n = lay[name]
            got, want = dbg[e, o:o + n], d.get(oname)
            worst[name] = max(worst.get(name, 0), _rel(got, want))
        active = d.get("con_dist") < 0
        nact += active.sum()
        # constraint rows of active contacts: D and aref (4 pyramid rows each)
        o, n = lay["con_D"]
        D = d.get("efc_D")[M.nlimit:].reshape(-1, 4)[:, 0]
        aref = d.get("efc_aref")[M.nlimit:].reshape(-1, 4)
        if active.any():
            worst["con_D"] = max(worst.get("con_D", 0), _rel(dbg[e, o:o + n][active], D[active]))
            o, n = lay["con_aref"]
            worst["con_aref"] = max(worst.get("con_aref", 0), _rel(dbg[e, o:o + n].reshape(-1, 4)[active], aref[active]))
    assert "lim_D" in worst and nlim > 0           # the scenario exercises joint limits too
    print("worst relative error per stage:", {k: f"{v:.2e}" for k, v in worst.items()}, "active contacts/env", nact / N)
    assert nact > N            # the scenario exercises contacts
    tol = {n: t for n, _, t in STAGES}
    tol.update(con_D=2e-4, con_aref=4e-5, lim_D=2e-4, lim_aref=4e-5)          # [3.6e-5, 7.0e-6]; limits: same formulas
    bad = {k: v for k, v in worst.items() if not v <= tol[k]}
    assert not bad, bad


def test_forward_stages_match_oracle_candidate_pairs(oracle_built):
    """rodent_cpu, the model with candidate-pair contacts, through the debug-dump instance of the DYN kernel: a sibling of the test above,
    because the model has no floor and no free joint (no settled states) and its contact sections are per candidate pair.  Colliding
    poses inside the joint limits (tests/pair_contact_cases.py); the STAGES bounds unchanged on every stage up to con_dist -- the
    hinge-root kinematics and the tendon transmission (qfrc_actuator) among them, and on con_pos of the pairs with a sphere and con_frame
    of the sphere-sphere pairs.  The rest of con_pos / con_frame, and the slots: tests/test_gpu_pair_contacts.py, under a criterion that
    knows the ill-conditioned capsule pairs (the float32 oracle itself is 7e-4 off on their normals).  The sections STAGES does not name are held to 3x the worse of the oracle's two float32 builds + 2^-22
    of the field's scale (the form of tests/smooth_regime.py); the limit rows and the solver's sections as in the tests around."""
    from rodent_amd import assets, hip
    from tests import pair_contact_cases as pc
    N = pc.N
    st, ctrl = pc.inputs("shipped", pc.MODEL, seed=5)
    st = pc.beyond_limits(st, seed=6)                           # three hinges per env past an end of their range: limit rows
    dev = torch.device("cuda:0")
    batch = hip.Batch(hip.Model(assets.asset_path(pc.MODEL), iterations=8, ls_iterations=8), N, dev)
    ds = _to_dev(st, dev)
    dbg = torch.zeros(N, batch.dims.dbg_floats, device=dev)
    batch.pipeline_step(ds, torch.tensor(ctrl, dtype=torch.float32, device=dev), 1, out=dict(debug=dbg))
    torch.cuda.synchronize()
    lay = batch.debug_layout()
    dbg = dbg.cpu().numpy().astype(np.float64)
    sec = lambda name: dbg[:, lay[name][0]:lay[name][0] + lay[name][1]]
    O = {p: pc.PairOracle(pc.MODEL, N, p).forward(st, ctrl) for p in ("f64", "f32", "f32fma")}
    A = O["f64"]
    m = pc.shipped()
    nb, nlimit = int(m["nbody"]), A.M.nlimit
    assert int((A.get("con_dist") < 0).sum()) > N               # the scenario exercises contacts
    worst = {}
    for name, oname, tol in STAGES:
        if name not in ("con_pos", "con_frame"):                # by kind, below
            worst[name] = max(_rel(sec(name)[e], A.get(oname)[e]) for e in range(N))
    tol = {n: t for n, _, t in STAGES}
    # con_pos / con_frame under their STAGES bounds where an independent float32 evaluation can meet them: the position of the pairs with a
    # sphere (kinds 4, 5), the frame of the sphere-sphere pairs (the float32 oracle: 1.4e-7 m, 6.2e-7; sphere-capsule frames 3.2e-6)
    kind, P = np.asarray(m["con_kind"]), A.M.ncon
    for name, width, kinds in (("con_pos", 3, (4, 5)), ("con_frame", 9, (4,))):
        g, w = sec(name).reshape(N, P, width)[:, np.isin(kind, kinds)], A.get(name).reshape(N, P, width)[:, np.isin(kind, kinds)]
        worst[name] = max(_rel(g[e], w[e]) for e in range(N))
    # rows of the pairs in penetration in both evaluations, by pair (condim 1: one row)
    wD, wa = A.rows(m)
    both = (A.get("con_dist") < -2e-6) & (sec("con_dist") < 0)
    assert both.sum() > N
    worst["con_D"], worst["con_aref"] = _rel(sec("con_D")[both], wD[both]), _rel(sec("con_aref").reshape(N, P, 4)[both], wa[both])
    tol.update(con_D=2e-4, con_aref=4e-5)
    # limit rows (every hinge is limited): activity exact away from the switching point, D / aref of the active rows
    lim_dof = m["jnt_dofadr"][m["limit_jnt"]]
    lim = sec("limit_pos_D_aref").reshape(N, -1, 3)[:, lim_dof]
    lpos = A.get("efc_pos")[:, :nlimit]
    assert np.array_equal((lim[:, :, 0] < 0)[np.abs(lpos) > 2e-6], (lpos < 0)[np.abs(lpos) > 2e-6])
    la = lpos < -2e-6
    assert la.sum() > N                                         # ... and joint limits (corner poses)
    worst["lim_D"] = _rel(lim[:, :, 1][la], A.get("efc_D")[:, :nlimit][la])
    worst["lim_aref"] = _rel(lim[:, :, 2][la], A.get("efc_aref")[:, :nlimit][la])
    tol.update(lim_D=2e-4, lim_aref=4e-5)
    # sections without a STAGES bound: the yardstick of the run
    root = A.get("subtree_com").reshape(N, nb, 3)[:, 1]
    extra = {"subtree_com": (sec("subtree_com")[:, :3], lambda o: o.get("subtree_com").reshape(N, nb, 3)[:, 1]),
             "cfrc": (sec("cfrc"), lambda o: np.concatenate([np.zeros((N, 6)), o.get("cfrc")[:, 6:]], 1)),
             "qLDiagInv": (sec("qLDiagInv"), lambda o: o.get("qLDiagInv"))}
    assert np.abs(root).max() > 0 and (sec("subtree_com")[:, 3:] == 0).all()      # one tree: the second tree's cells hold 0
    for name, (got, f) in extra.items():
        want = f(A)
        scale = np.abs(want).max()
        worst[name] = np.abs(got - want).max() / scale
        tol[name] = 3.0 * max(np.abs(f(O[p]) - want).max() / scale for p in ("f32", "f32fma")) + 2.0 ** -22
    # the solver's sections: qacc is what the launch hands on, bit for bit; bounds of test_solver_and_substep_match_oracle below
    assert np.array_equal(sec("qacc").astype(np.float32), ds["qacc_warmstart"].cpu().numpy())
    # ... and, like qfrc_constraint, the result of a truncated CG run with rows active: heavy-tailed against float64 whoever computes it
    # (tests/parity.py), so by C3 -- the median and the 90th percentile of the per-env error within 3x the worse float32 build's + floor
    from tests import parity
    niter, rows = sec("niter_cost")[:, 0], []
    # floors as parity.SUBSTEP_FLOORS["qacc"]: a few float32 ulps of a quantity scaled to 1 (each of these errors is divided by its env's scale)
    floors = dict(qacc=parity.SUBSTEP_FLOORS["qacc"], qfrc_constraint=2e-6, solver_cost=2e-6)
    dumped = dict(qacc=sec("qacc"), qfrc_constraint=sec("qfrc_constraint"), solver_cost=sec("niter_cost")[:, 1:2])
    for name, floor_scale in (("qacc", 1.0), ("qfrc_constraint", 1e-3), ("solver_cost", 1.0)):
        want = A.get(name).reshape(N, -1)
        sc = np.maximum(np.abs(want).max(1), floor_scale)
        gaps = [np.abs(O[p].get(name).reshape(N, -1) - want).max(1) / sc for p in ("f32", "f32fma")]
        for q in (0.5, 0.9):
            rows.append((name, q, float(np.quantile(np.abs(dumped[name] - want).max(1) / sc, q)), max(float(np.quantile(g, q)) for g in gaps)))
    print("worst relative error per stage:", {k: f"{v:.2e} ({tol[k]:.1e})" for k, v in worst.items()}, "| (section, q, err, float32 oracle)", rows)
    parity.check_quantiles(rows, floors)
    print("iteration count against the float32 oracle's where float64 iterates: equal, within one",
          pc.assert_iteration_counts(niter, A.get("solver_niter")[:, 0], O["f32"].get("solver_niter")[:, 0]))      # C2 on this model
    assert (sec("kernarg_ok") == 1).all()
    ls, end = sec("ls_iters"), sec("solver_end").astype(int)
    assert (ls >= 0).all() and (ls == np.round(ls)).all()
    # solver_end: [0] which start was chosen; [1] how the loop ended, a sum of 1 (iteration cap), 2 (improvement), 4 (gradient): never 0
    assert np.isin(end[:, 0], (0, 1)).all() and (end[:, 1] >= 1).all() and (end[:, 1] <= 7).all()
    assert np.array_equal(end[:, 1] & 1, (niter >= 8).astype(int))
    bad = {k: v for k, v in worst.items() if not v <= tol[k]}
    assert not bad, bad


@pytest.mark.parametrize("model,instance", [("rodent_optimized", "debug_dump"), ("rodent_optimized", "production"),
                                            ("rodent_new", "production"), ("rodent_pair", "production")])
def test_solver_and_substep_match_oracle(oracle_built, model, instance):
    """qacc after the CG solve and qpos/qvel after one substep, same inputs (float32 vs float64 oracle), for both kernel
    instances: the debug-dump instance (generic dimensions) that the stage tests read, and the production instances (no
    dump; fixed dimensions for rodent_optimized -- the one that is timed -- and generic ones for the other models).  The two differ in instruction selection (constant folding / FMA
    contraction), so their outputs differ at rounding level; each must meet the same bounds against the oracle."""
    from rodent_amd import assets, hip
    ref = oracle_built
    N = 48 if model == "rodent_optimized" else 16
    st, M, m = util.settled_states(ref, model, N, seed=2, iterations=(8, 8))
    dev = torch.device("cuda:0")
    batch = hip.Batch(hip.Model(assets.asset_path(model), 8, 8), N, dev)
    ctrl = np.random.default_rng(6).uniform(-1, 1, (N, M.nu))
    ds = _to_dev(st, dev)
    dbg = torch.zeros(N, batch.dims.dbg_floats, device=dev)
    batch.pipeline_step(ds, torch.tensor(ctrl, dtype=torch.float32, device=dev), 1,
                        out=dict(debug=dbg) if instance == "debug_dump" else None)
    torch.cuda.synchronize()
    lay = batch.debug_layout()
    dbg = dbg.cpu().numpy().astype(np.float64)
    got_qacc = ds["qacc_warmstart"].cpu().numpy().astype(np.float64)      # the warm start handed on IS the solver's qacc
    err_qacc, err_qvel, err_qpos, err_f = [], [], [], []
    for e in range(N):
        d = util.oracle_forward(ref, M, st, e, ctrl[e])
        qacc = d.get("qacc")
        err_qacc.append(np.abs(got_qacc[e] - qacc).max() / max(np.abs(qacc).max(), 1.0))
        if instance == "debug_dump":
            o, n = lay["qacc"]
            np.testing.assert_array_equal(dbg[e, o:o + n].astype(np.float32), got_qacc[e].astype(np.float32))
            o, n = lay["qfrc_constraint"]
            fc = d.get("qfrc_constraint")
            err_f.append(np.abs(dbg[e, o:o + n] - fc).max() / max(np.abs(fc).max(), 1e-3))
        d2 = ref.RefData(M)
        for k in ("qpos", "qvel", "act", "qacc_warmstart"):
            d2.set(k, st[k][e])
        d2.step(ctrl[e], 1)
        dv = np.abs(d2.get("qvel") - st["qvel"][e]).max()           # scale: the substep's velocity change
        err_qvel.append(np.abs(ds["qvel"][e].cpu().numpy() - d2.get("qvel")).max() / max(dv, 1e-3))
        err_qpos.append(np.abs(ds["qpos"][e].cpu().numpy() - d2.get("qpos")).max())
    print(model, "%s: qacc rel err: median %.2e max %.2e | qvel err / max|dqvel| max %.2e | qpos abs max %.2e"
          % (instance, np.median(err_qacc), np.max(err_qacc), np.max(err_qvel), np.max(err_qpos)))
    # a truncated (8-iteration) CG run in float32 vs float64: branchy line search -> allow a few outliers
    # <= 10x the worst value measured on MI355X in round 1 [median 1.2e-6, max 4.0e-5 | 3.4e-4 | 2.0e-5 | 7.0e-4]
    assert np.median(err_qacc) < 1e-5
    assert np.max(err_qacc) < 4e-4
    if err_f:
        assert np.max(err_f) < 3e-3
    assert np.max(err_qpos) < 1e-4
    assert np.median(err_qvel) < 1e-4 and np.max(err_qvel) < 5e-3
