"""The candidate-pair contact code of the step kernel (rodent_cpu, the DYN instances) read back through its debug-dump instance:
pair_geometry / seg_point / seg_seg per pair, the compaction of the pairs in penetration into the 64 slots, the drop-and-flag path
beyond them, and the rows of the slotted pairs (signed dof chains, condim 1 and 3) -- against the float64 oracle, on the shipped blob
and on the radius-scaled variants of tests/pair_contact_cases.py, whose criterion tests/test_pair_contacts_cpu.py validates.

64 envs, one substep per launch, float32-rounded inputs; every case's oracle results and launches are made once (fixture `runs`)."""
import numpy as np
import pytest
import torch

from tests import pair_contact_cases as pc
from tests import parity
from tests.hip_impl import HipImpl, NoDiscrete

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("shipped", "dense", "spheres", "overflow")
GEOMETRY_CASES = ("shipped", "dense", "spheres")
ROW_CASES = ("dense", "spheres")


def _launch(impl, st, ctrl, n_frames=1, debug=True):
    """One launch: (state after, dump by section or None, contact outputs or None)."""
    b, n, d = impl.batch, impl.n, impl.batch.dims
    ds = impl._dev(st)
    out = None
    if debug:
        out = dict(debug=torch.full((n, d.dbg_floats), float("nan"), device=DEV), contact_dist=torch.zeros(n, d.ncon, device=DEV),
                   contact_pos=torch.zeros(n, 3 * d.ncon, device=DEV), contact_frame=torch.zeros(n, 9 * d.ncon, device=DEV))
    b.pipeline_step(ds, torch.tensor(ctrl, dtype=torch.float32, device=DEV), n_frames, out=out)
    torch.cuda.synchronize()
    state = {k: v.cpu().numpy() for k, v in ds.items()}
    if not debug:
        return state, None, None
    g = out["debug"].cpu().numpy()
    return state, {k: g[:, o:o + w] for k, (o, w) in impl.lay.items()}, {k: v.cpu().numpy() for k, v in out.items() if k != "debug"}


@pytest.fixture(scope="module")
def runs(oracle_built, tmp_path_factory):
    folder = tmp_path_factory.mktemp("pair_blobs")
    out = {}
    for case in CASES:
        m, stem = pc.variant(case), pc.blob(case, folder)
        st, ctrl = pc.inputs(case, stem)
        A = pc.PairOracle(stem, pc.N, "f64").forward(st, ctrl)
        pc.assert_regime(case, A.get("con_dist"))              # before anything is compared
        cond = pc.conditioning(m, A.get("geom_xpos").reshape(pc.N, -1, 3), A.get("geom_xmat"))
        ys = [pc.PairOracle(stem, pc.N, p).forward(st, ctrl).geometry() for p in ("f32", "f32fma")]
        impl = HipImpl(stem, pc.N, (8, 8), True)
        state, dump, outs = _launch(impl, st, ctrl)
        P = impl.batch.dims.ncon
        got = dict(dist=dump["con_dist"].astype(np.float64), pos=dump["con_pos"].astype(np.float64).reshape(pc.N, P, 3),
                   frame=dump["con_frame"].astype(np.float64).reshape(pc.N, P, 9))
        out[case] = dict(m=m, stem=stem, st=st, ctrl=ctrl, A=A, want=A.geometry(), rows=A.rows(m), keep=pc.kept_samples(cond), ys=ys, impl=impl,
                         state=state, dump=dump, outs=outs, got=got)
    return out


@pytest.mark.parametrize("case", CASES)
def test_dump_layout_and_contact_outputs(runs, case):
    """The sections are those of pair_contact_cases.dyn_sections, every cell of the dump was written (it was NaN before the launch), the
    kernel saw its own I/O block, and rr_outputs' three contact arrays hold the dump's values bit for bit."""
    r = runs[case]
    impl, dump = r["impl"], r["dump"]
    o = 0
    assert list(impl.lay) == [n for n, _ in pc.dyn_sections(impl.batch.dims)]
    for name, w in pc.dyn_sections(impl.batch.dims):
        assert impl.lay[name] == (o, w), name
        o += w
    assert o == impl.batch.dims.dbg_floats
    lim = np.zeros((impl.batch.dims.nv, 3), bool)
    lim[impl.lim_dof] = True                      # limit_pos_D_aref: the rows of the limited dofs (every hinge of this model)
    for name, v in dump.items():
        written = np.isfinite(v) if name != "limit_pos_D_aref" else np.isfinite(v) | ~lim.reshape(-1)[None]
        assert written.all(), (name, np.argwhere(~written)[:5])
    assert (dump["kernarg_ok"] == 1).all()
    for k, sec in (("contact_dist", "con_dist"), ("contact_pos", "con_pos"), ("contact_frame", "con_frame")):
        assert np.array_equal(r["outs"][k].view(np.int32), dump[sec].view(np.int32)), k


@pytest.mark.parametrize("case", GEOMETRY_CASES)
def test_per_pair_geometry(runs, case):
    """All 2243 pairs of every env: activity, and per kind the largest error of dist (all pair-samples) and of pos / normal / tangents
    (the well-conditioned ones) within 3 x the worse float32 oracle build's + 2^-22 of the field's magnitude."""
    r = runs[case]
    shares = pc.excluded_shares(r["m"], r["keep"])
    assert max(shares.values()) <= pc.MAX_EXCLUDED, shares
    rec, bad = pc.judge(r["m"], r["got"], r["want"], r["ys"], r["keep"])
    print(case + "\n" + pc.report(rec))
    assert not bad, bad


@pytest.mark.parametrize("case", CASES)
def test_slots_hold_the_penetrating_pairs_in_list_order(runs, case):
    r = runs[case]
    dump, want = r["dump"], r["want"]["dist"]
    slot, count = dump["slot_pair"].astype(int), dump["pen_count"][:, 0].astype(int)
    D, aref = dump["con_D"], dump["con_aref"].reshape(pc.N, -1, 4)
    agree = 0
    for e in range(pc.N):
        pen = np.nonzero(dump["con_dist"][e] < 0)[0]              # the kernel's own distances: what it dumped is what selected
        assert count[e] == len(pen), (e, count[e], len(pen))
        k = min(len(pen), pc.SLOTS)
        assert np.array_equal(slot[e, :k], pen[:k]) and (slot[e, k:] == -1).all(), e
        free = np.ones(D.shape[1], bool)
        free[pen[:k]] = False
        assert (D[e, free] == 0).all() and (aref[e, free] == 0).all() and (D[e, pen[:k]] > 0).all(), e
        if not (np.abs(want[e]) < pc.EDGE).any():
            wpen = np.nonzero(want[e] < 0)[0]
            assert count[e] == len(wpen) and np.array_equal(pen[:k], wpen[:k]), e
            agree += 1
    assert agree >= pc.N // 2, agree              # envs with a pair within EDGE of zero are the exception
    if case == "overflow":
        assert (count > pc.SLOTS).all()
    else:
        assert (count <= pc.SLOTS).all() and r["impl"].batch.contact_overflow() == 0


def test_rows_of_the_slotted_pairs(runs):
    """con_D and con_aref of the pairs in a slot against the oracle's efc_D / efc_aref of the same pairs: all four pyramid rows of a
    condim-3 pair (the signed chains of J = jac(body2) - jac(body1), friction directions included -- qvel is not zero), row 0 of a
    condim-1 pair, whose other rows are 0.  Bounds as in test_gpu_parity.py: 2e-4 / 4e-5 of the field's scale."""
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    seen_kind, seen_dim = set(), set()
    for case in ROW_CASES:
        r = runs[case]
        kind, dims = np.asarray(r["m"]["con_kind"]), np.asarray(r["m"]["con_dim"])
        wD, wa = r["rows"]
        D, aref = r["dump"]["con_D"].astype(np.float64), r["dump"]["con_aref"].astype(np.float64).reshape(pc.N, -1, 4)
        both = (r["want"]["dist"] < -pc.EDGE) & (r["dump"]["con_dist"] < 0)          # a row in both evaluations
        assert both.sum() >= 20 * pc.N
        for dim in (1, 3):
            sel = both & (dims == dim)[None]
            assert sel.any(), (case, dim)
            eD, ea = rel(D[sel], wD[sel]), rel(aref[sel], wa[sel])
            print(case, "condim", dim, "rows of", int(sel.sum()), "pair-samples: con_D %.2e con_aref %.2e" % (eD, ea))
            assert eD <= 2e-4 and ea <= 4e-5, (case, dim, eD, ea)
            if dim == 1:
                assert (aref[sel][:, 1:] == 0).all() and (np.abs(wa[sel][:, 0]) > 0).any()
            else:
                assert (np.abs(wa[sel][:, 1:] - wa[sel][:, :1]).max(0) > 0).all()     # the friction rows do differ from one another
            seen_dim.add(dim)
        seen_kind |= set(kind[both.any(0)].tolist())
    assert seen_kind == {4, 5, 6} and seen_dim == {1, 3}, (seen_kind, seen_dim)


def test_overflow_drops_counts_and_stays_deterministic(runs):
    """More than 64 pairs in penetration in every env: the first 64 in list order are kept (test_slots...), the counter rises by one per
    (env, env step) whatever the number of substeps, the state stays finite and two launches give the same bits.  No comparison of the
    dynamics with the oracle: it drops nothing."""
    r = runs["overflow"]
    impl = r["impl"]
    assert (r["dump"]["pen_count"][:, 0] > pc.SLOTS).all()
    base = impl.batch.contact_overflow()
    s1, d1, _ = _launch(impl, r["st"], r["ctrl"])
    assert impl.batch.contact_overflow() == base + pc.N
    s3, _, _ = _launch(impl, r["st"], r["ctrl"], n_frames=3, debug=False)
    assert impl.batch.contact_overflow() == base + 2 * pc.N
    s3b, _, _ = _launch(impl, r["st"], r["ctrl"], n_frames=3, debug=False)
    for a, b in ((s1, r["state"]), (s3, s3b)):
        assert all(np.isfinite(a[k]).all() and np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)
    assert all(np.array_equal(d1[k].view(np.int32), r["dump"][k].view(np.int32)) for k in d1)


def test_debug_and_production_instances_meet_the_substep_criteria(oracle_built):
    """The same inputs through the debug-dump instance and the production single-step DYN instance: each meets the substep criteria of
    tests/parity.py against the float64 oracle (they differ in instruction selection, so not bit for bit) -- the debug instance with
    its own con_dist, limit rows and iteration count (C2 in the form of pair_contact_cases.assert_iteration_counts), the production one, which
    has none to show, on the state criteria."""
    seq = [(pc.beyond_limits(st, s), c) for s in (21, 22, 23, 24) for st, c in [pc.inputs("shipped", pc.MODEL, seed=s)]]      # with limit rows
    A = parity.OracleImpl(pc.MODEL, pc.N, "f64", (8, 8))
    B = parity.OracleImpl(pc.MODEL, pc.N, "f32", (8, 8))
    assert sum(int((A.substep(st, c)["con_dist"] < 0).sum()) for st, c in seq) >= 2 * pc.N
    impl, RA, RB = pc.Recording(HipImpl(pc.MODEL, pc.N, (8, 8), True)), pc.Recording(A), pc.Recording(B)
    dbg = parity.substep_ladder(impl, seq, RA, RB)
    print("debug", dbg["quantiles"], "niter equal", dbg["niter_equal"], "(float32 oracle: %g)" % dbg["niter_equal_f32_oracle"], dbg["limit_rows"])
    assert dbg["limit_rows"]["lim_D"] > 0                   # limit rows were active
    print("iteration count against the float32 oracle's where float64 iterates: equal, within one", pc.assert_substep_criteria(dbg, impl, RA, RB))
    prod = parity.substep_ladder(NoDiscrete(HipImpl(pc.MODEL, pc.N, (8, 8), False), A), seq, A, B)
    print("production", prod["quantiles"])
    parity.check_quantiles(prod["quantiles"], parity.SUBSTEP_FLOORS)
