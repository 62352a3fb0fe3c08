"""Candidate-pair contacts of rodent_cpu (the DYN instances of the step kernel): the blob variants that reach what the shipped model
within its joint limits does not, their inputs, and the per-pair criterion ("Per-pair contact parity").

Shared by tests/test_pair_contacts_cpu.py (regime facts, exclusion caps, the criterion on the oracle's float32 builds and on seeded
errors) and tests/test_gpu_pair_contacts.py (the debug-dump instance of the kernel).

Variants.  A variant is rodent_cpu.rrm with geom_size[:, 0] (the radius) of some sphere / capsule geoms multiplied by a factor, and the
kernel tables rebuilt -- k_con_f from the edited sizes.  Nothing else changes.
  shipped   the blob as it is: 0.5 pairs in penetration per random pose, never a sphere-sphere pair
  dense     every radius x 1.5, poses kept at <= 64 pairs in penetration: tens of contacts of both condims per env
  spheres   the spheres of the 18 sphere-sphere pairs x SPHERES_FACTOR: sphere-sphere contacts, no overflow
  overflow  every radius x 3: more than 64 pairs in penetration in every env

Criterion (per kind 4 / 5 / 6 and field dist / pos / normal / tangents), on pair-samples = (env, pair):
  activity   sign(dist) equals the float64 oracle's unless |dist64| < EDGE                               (C1 of tests/parity.py)
  error      max over the kept pair-samples of |x - f64|  <=  3 * the same maximum of the worse of the oracle's f32 and f32fma builds
             + 2^-22 * the field's largest magnitude
  kept       dist: every pair-sample.  pos, normal, tangents: the samples that pass the conditioning filter below, which reads float64
             quantities alone (the oracle's geom poses); at most MAX_EXCLUDED of a kind's samples may fail it."""
import numpy as np

from oracle import ref
from rodent_amd import assets, ktables, mjcf
from tests import smooth_regime as sr

MODEL = "rodent_cpu"
N = 64
SLOTS = 64
EDGE = 2e-6
FACTOR, FLOOR = 3.0, 2.0 ** -22
MAX_EXCLUDED = 0.01
KINDS = (4, 5, 6)
FIELDS = ("dist", "pos", "normal", "tangents")
SPHERES_FACTOR = 4.0
# The conditioning filter.  THETA: capsule-capsule pairs need 1 - (a1.a2)^2 >= THETA (the line solve's denominator).  RHO, DELTA: where the
# two re-projection candidates lie more than DELTA apart, their squared distances must differ by RHO of the larger (else a float32
# evaluation may keep the other one).  ELL: the closest points must be ELL apart (the normal is their difference, normalised).
# NY: ||n_y| - 0.5| >= NY for the tangents (make_frame switches its seed vector at |n_y| = 0.5).
THETA, RHO, DELTA, ELL, NY = 1e-4, 1e-4, 1e-6, 1e-4, 1e-4


def f32r(x):
    return sr.f32r(x)


# ------------------------------------------------------------------------------------------ variants
def shipped():
    return mjcf.load_blob(assets.asset_path(MODEL))


def sphere_pair_geoms(m):
    """The geoms of the sphere-sphere candidate pairs."""
    k4 = np.asarray(m["con_kind"]) == 4
    return np.unique(np.concatenate([np.asarray(m["con_geom1"])[k4], np.asarray(m["con_geom2"])[k4]]))


def scaled_variant(m, factor, geoms=None):
    """`m` with the radius of its sphere and capsule geoms (of `geoms` among them, if given) times `factor`, tables rebuilt."""
    out = dict(m)
    size = np.array(m["geom_size"], copy=True)
    gt = np.asarray(m["geom_type"])
    sel = (gt == mjcf.SPHERE) | (gt == mjcf.CAPSULE)
    if geoms is not None:
        sel &= np.isin(np.arange(len(gt)), geoms)
    size[sel, 0] = (size[sel, 0].astype(np.float64) * factor).astype(size.dtype)
    out["geom_size"] = size
    return retabled(out)


def retabled(out):
    """The kernel tables of the edited raw fields `out`.  sr.rebuild_tables leaves k_con_f as shipped (KEPT_TABLES); here it carries the
    edit, so it comes from the same build."""
    md = {k: (np.asarray(v, np.float64) if np.asarray(v).dtype.kind == "f" else np.asarray(v)) for k, v in out.items()}
    with sr._shipped_schedules():
        kt = ktables.build_kernel_tables(md)
    out = dict(out)
    out.update({k: sr.stored(v).reshape(np.shape(out[k])) for k, v in kt.items() if k in out and k not in ("h_k_con_f",)})
    return out


def variant(case, m=None):
    m = shipped() if m is None else m
    if case == "shipped":
        return m
    if case == "dense":
        return scaled_variant(m, 1.5)
    if case == "spheres":
        return scaled_variant(m, SPHERES_FACTOR, sphere_pair_geoms(m))
    if case == "overflow":
        return scaled_variant(m, 3.0)
    raise KeyError(case)


def blob(case, folder):
    """-> the stem (path without '.rrm') of the case's blob; the shipped model's own path for `shipped`."""
    if case == "shipped":
        return MODEL
    return sr.write_blob(variant(case), folder, f"{MODEL}_{case}")


# ------------------------------------------------------------------------------------------ inputs
def poses(m, n, rng, corner):
    """[n, nq] hinge angles inside the limits: random (qpos0 + s U(lo, hi), s ~ U(0.2, 1)) or corner poses (every joint 2 % of its range
    from one of its ends, the end drawn per joint)."""
    lo, hi = np.asarray(m["jnt_range"], np.float64)[:, 0], np.asarray(m["jnt_range"], np.float64)[:, 1]
    if corner:
        t = np.where(rng.integers(0, 2, (n, len(lo))) == 1, 0.98, 0.02)
        return lo + (hi - lo) * t
    return np.asarray(m["qpos0"], np.float64) + rng.uniform(0.2, 1.0, (n, 1)) * rng.uniform(lo, hi, (n, len(lo)))


def inputs(case, stem, n=N, seed=0):
    """(state, ctrl) of a case, float32-rounded: half random and half corner poses, drawn until `n` pass the case's pose filter on the
    float64 oracle (dense, spheres: at most SLOTS pairs in penetration; spheres: the poses with a sphere-sphere pair active first);
    qvel ~ U(-0.5, 0.5), act ~ U(-0.5, 0.5), ctrl ~ U(-1, 1), qacc_warmstart 0."""
    m = shipped()
    M = ref.RefModel(assets.asset_path(stem), "f64")
    d = ref.RefData(M)
    rng = np.random.default_rng(seed)
    kind = np.asarray(m["con_kind"])
    keep, extra, draws = [], [], 0
    while len(keep) < n and draws < 40 * n:
        q = f32r(poses(m, 1, rng, corner=draws % 2 == 1)[0])
        draws += 1
        d.init(q, np.zeros(M.nv))
        dist = d.get("con_dist")
        npen = int((dist < 0).sum())
        if case in ("dense", "spheres") and npen > SLOTS:
            continue
        if case == "spheres" and not (dist[kind == 4] < 0).any():
            if len(extra) < n // 2:
                extra.append(q)
            continue
        keep.append(q)
    if case == "spheres":
        keep = (keep + extra)[:n]
    assert len(keep) == n, (case, len(keep), draws)
    st = dict(qpos=np.asarray(keep), qvel=rng.uniform(-0.5, 0.5, (n, M.nv)), act=rng.uniform(-0.5, 0.5, (n, M.nu)), qacc_warmstart=np.zeros((n, M.nv)))
    return {k: f32r(v) for k, v in st.items()}, f32r(rng.uniform(-1, 1, (n, M.nu)))


def beyond_limits(st, seed, joints=3, by=0.02):
    """`st` with `joints` hinges per env moved `by` of their range past one of its ends (float32-rounded): limit rows that are active."""
    m = shipped()
    lo, hi = np.asarray(m["jnt_range"], np.float64)[:, 0], np.asarray(m["jnt_range"], np.float64)[:, 1]
    rng = np.random.default_rng(seed)
    q = st["qpos"].copy()
    for e in range(len(q)):
        for j in rng.choice(len(lo), joints, replace=False):
            q[e, j] = lo[j] - by * (hi[j] - lo[j]) if rng.integers(0, 2) else hi[j] + by * (hi[j] - lo[j])
    return dict(st, qpos=f32r(q))


def assert_regime(case, dist):
    """The case is in the regime it claims: `dist` [n, P] of the float64 oracle on its inputs."""
    m = shipped()
    kind, dims = np.asarray(m["con_kind"]), np.asarray(m["con_dim"])
    pen = dist < 0
    if case == "shipped":
        assert pen.sum(1).max() <= SLOTS and not pen[:, kind == 4].any()          # what the variants are for
    elif case == "dense":
        assert pen.sum(1).max() <= SLOTS and pen.sum(1).mean() >= 20 and pen[:, dims == 1].any() and pen[:, dims == 3].any()
    elif case == "spheres":
        assert pen.sum(1).max() <= SLOTS and int(pen[:, kind == 4].sum()) >= 10
    elif case == "overflow":
        for e, row in enumerate(dist):
            assert int((row < -EDGE).sum()) > SLOTS, e
            first = np.nonzero(row < 0)[0][:SLOTS + 1]             # the first 65 in list order, and nothing near zero before the last of them
            assert (np.abs(row[first]) >= EDGE).all() and not (np.abs(row[:first[-1]]) < EDGE).any(), e
    else:
        raise KeyError(case)


# ------------------------------------------------------------------------------------------ oracle
class PairOracle:
    """n envs of the oracle on a blob in one precision: one forward pass, the per-pair fields and the rows."""

    def __init__(self, stem, n, precision, iterations=(8, 8)):
        self.M = ref.RefModel(assets.asset_path(stem), precision)
        self.M.set_iterations(*iterations)
        self.b = ref.RefBatch(self.M, n)
        self.n = n

    def forward(self, st, ctrl):
        self.b.set_state(st)
        for e, d in enumerate(self.b.d):
            d.set("ctrl", ctrl[e])
            d.forward()
        return self

    def get(self, name):
        return self.b.get(name)

    def geometry(self):
        """dist [n, P], pos [n, P, 3], frame [n, P, 9] (normal, two tangents) of the last forward pass."""
        P = self.M.ncon
        return dict(dist=self.get("con_dist"), pos=self.get("con_pos").reshape(self.n, P, 3), frame=self.get("con_frame").reshape(self.n, P, 9))

    def rows(self, m):
        """(D [n, P], aref [n, P, 4]) of the contact rows by pair: a condim-1 pair has one row (the other three 0), a condim-3 pair four."""
        dims = np.asarray(m["con_dim"])
        nl = self.M.nlimit
        row_of = nl + np.concatenate([[0], np.cumsum(np.where(dims == 1, 1, 4))[:-1]])
        eD, ea = self.get("efc_D"), self.get("efc_aref")
        D = eD[:, row_of]
        aref = np.zeros((self.n, len(dims), 4))
        for k in range(4):
            has = (dims == 3) | (k == 0)
            aref[:, has, k] = ea[:, row_of[has] + k]
        return D, aref


# ------------------------------------------------------------------------------------------ the conditioning filter (float64 only)
def _dot(a, b):
    return (a * b).sum(-1)


def _seg_point(a, b, pt):
    ab = b - a
    t = np.clip(_dot(pt - a, ab) / (_dot(ab, ab) + 1e-6), 0.0, 1.0)
    return a + ab * t[..., None]


def conditioning(m, geom_xpos, geom_xmat):
    """Float64 geometry of every pair-sample from the oracle's geom poses (geom_xpos [n, G, 3], geom_xmat [n, G, 9]) and the blob's sizes,
    in numpy: -> dict(dist, par = 1 - (a1.a2)^2, margin = |e1 - e2| / max(e1, e2) of the two re-projection candidates' squared distances,
    apart = how far the two candidates lie from each other, sep = the closest points' separation, ny = the normal's y).  The formulas are
    those of oracle/np_ref.py (_segment_point, _segment_segment, _two_spheres), over all samples at once."""
    g1, g2, kind = np.asarray(m["con_geom1"]), np.asarray(m["con_geom2"]), np.asarray(m["con_kind"])
    size = np.asarray(m["geom_size"], np.float64)
    n = geom_xpos.shape[0]
    xm = geom_xmat.reshape(n, -1, 3, 3)
    P1, P2 = geom_xpos[:, g1], geom_xpos[:, g2]
    ax1, ax2 = xm[:, g1][..., 2], xm[:, g2][..., 2]                   # third column: the capsule axis
    h1, h2 = size[g1, 1][None, :, None], size[g2, 1][None, :, None]
    k5, k6 = (kind == 5)[None, :, None], (kind == 6)[None, :, None]
    # kind 5: the closest point of capsule 2's segment to sphere 1's centre
    b5 = _seg_point(P2 - ax2 * h2, P2 + ax2 * h2, P1)
    # kind 6: the regularised line solve from the mid-points, clipped, and the two re-projection candidates
    tr = P1 - P2
    c = _dot(ax1, ax2)
    ta = (-_dot(ax1, tr) + c * _dot(ax2, tr)) / (1 - c * c + 1e-6)
    tb = _dot(ax2, tr) + ta * c
    pa = P1 + ax1 * np.clip(ta, -h1[..., 0], h1[..., 0])[..., None]
    pb = P2 + ax2 * np.clip(tb, -h2[..., 0], h2[..., 0])[..., None]
    na, nb = _seg_point(P1 - ax1 * h1, P1 + ax1 * h1, pb), _seg_point(P2 - ax2 * h2, P2 + ax2 * h2, pa)
    e1, e2 = _dot(na - pb, na - pb), _dot(nb - pa, nb - pa)
    first = (e1 < e2)[..., None]
    a6, b6 = np.where(first, na, pa), np.where(first, pb, nb)
    a = np.where(k6, a6, P1)
    b = np.where(k6, b6, np.where(k5, b5, P2))
    v = b - a
    sep = np.sqrt(_dot(v, v))
    nrm = np.where(sep[..., None] > 0, v / np.where(sep > 0, sep, 1.0)[..., None], np.array([1.0, 0.0, 0.0]))
    is6 = kind == 6
    return dict(dist=sep - (size[g1, 0] + size[g2, 0])[None], par=np.where(is6, 1 - c * c, 1.0),
                margin=np.where(is6, np.abs(e1 - e2) / np.maximum(np.maximum(e1, e2), 1e-300), 1.0),
                apart=np.where(is6, np.maximum(np.sqrt(_dot(na - pa, na - pa)), np.sqrt(_dot(nb - pb, nb - pb))), 0.0),
                sep=sep, ny=nrm[..., 1])


def kept_samples(cond):
    """field -> bool [n, P]: the pair-samples the error bound covers."""
    well = (cond["par"] >= THETA) & ((cond["margin"] >= RHO) | (cond["apart"] <= DELTA)) & (cond["sep"] >= ELL)
    return dict(dist=np.ones_like(well), pos=well, normal=well, tangents=well & (np.abs(np.abs(cond["ny"]) - 0.5) >= NY))


def excluded_shares(m, keep):
    """(kind, field) -> share of the kind's pair-samples the filter leaves out."""
    kind = np.asarray(m["con_kind"])
    return {(k, f): float(1.0 - keep[f][:, kind == k].mean()) for k in KINDS for f in FIELDS}


# ------------------------------------------------------------------------------------------ the criterion
def errors(x, want):
    """field -> |x - want| per pair-sample (the largest component of the field)."""
    return dict(dist=np.abs(x["dist"] - want["dist"]), pos=np.abs(x["pos"] - want["pos"]).max(-1),
                normal=np.abs(x["frame"][..., :3] - want["frame"][..., :3]).max(-1),
                tangents=np.abs(x["frame"][..., 3:] - want["frame"][..., 3:]).max(-1))


def magnitudes(want):
    return dict(dist=np.abs(want["dist"]), pos=np.abs(want["pos"]).max(-1), normal=np.abs(want["frame"][..., :3]).max(-1),
                tangents=np.abs(want["frame"][..., 3:]).max(-1))


def judge(m, cand, want, yardsticks, keep):
    """-> (record, failures).  record[(kind, field)] = dict(err, yard=[..], bound, kept, worst=(env, pair)); failures: what misses the
    activity or the error criterion, as strings."""
    kind = np.asarray(m["con_kind"])
    rec, bad = {}, []
    flip = ((cand["dist"] < 0) != (want["dist"] < 0)) & (np.abs(want["dist"]) >= EDGE)
    if flip.any():
        bad.append("activity: %d pair-samples differ away from the switching point, first %s" % (int(flip.sum()), np.argwhere(flip)[:3].tolist()))
    for f in ("dist", "pos", "frame"):
        if not np.isfinite(cand[f]).all():
            bad.append(f + ": not finite")
    err, mag, ys = errors(cand, want), magnitudes(want), [errors(y, want) for y in yardsticks]
    for k in KINDS:
        for f in FIELDS:
            sel = keep[f] & (kind == k)[None]
            if not sel.any():
                bad.append(f"kind {k} {f}: no sample kept")
                continue
            e = np.where(sel, err[f], 0.0)
            yard = [float(y[f][sel].max()) for y in ys]
            bound = FACTOR * max(yard) + FLOOR * float(mag[f][sel].max())
            w = np.unravel_index(int(e.argmax()), e.shape)
            rec[(k, f)] = dict(err=float(e.max()), yard=yard, bound=bound, kept=int(sel.sum()), worst=(int(w[0]), int(w[1])))
            if not e.max() <= bound:
                bad.append(f"kind {k} {f}: {e.max():.3e} > {bound:.3e} at (env, pair) {rec[(k, f)]['worst']}")
    return rec, bad


def report(rec):
    return "\n".join("kind %d %-8s err %.2e  f32 %.2e  f32fma %.2e  bound %.2e  kept %d" % (k, f, r["err"], r["yard"][0], r["yard"][1], r["bound"], r["kept"])
                     for (k, f), r in rec.items())


# ------------------------------------------------------------------------------------------ the substep criteria on this model
class Recording:
    """An impl of parity.substep_ladder that keeps what its substeps returned (the iteration counts, sample by sample)."""

    def __init__(self, impl):
        self.impl, self.outs = impl, []

    def substep(self, st, ctrl):
        self.outs.append(self.impl.substep(st, ctrl))
        return self.outs[-1]

    def niter(self):
        return np.concatenate([o["niter"] for o in self.outs])


def assert_iteration_counts(got, f64, f32):
    """C2 on this model, in the form tests/parity.py gives it for the Newton solver.  `got`, `f64`, `f32`: iteration counts per sample of the
    implementation and of the oracle's float64 and float32 builds.

    Why not `equal to float64's in 90 %`.  On the floor-contact models nearly every sample ends at the iteration cap.  Here, with a handful
    of rows, the float64 run ends on its GRADIENT test: after the line search that reaches the minimum, |grad| is double round-off, below
    the tolerance, and it stops -- after 1 iteration in 19 of 119 and 45 of 191 iterating samples of the two ladders below.  A float32
    run's |grad| levels off at float32 rounding, above the tolerance; it takes one more line search, whose improvement is nil, and stops on
    the IMPROVEMENT test (the kernel's `solver_end` says so: every one of its stops between 2 and 7 iterations is an improvement stop, none
    a gradient stop).  So every float32 evaluation is one iteration late where float64 stops early: of the samples float64 ends in 1..7
    iterations the oracle's f32 / f32fma builds agree with it in 12 % to 14 %, the kernel in 13 % to 16 % (at the cap: 79 % to 94 %, all
    three alike), and overall none of the three is within one iteration of float64 in 99 %.  Measured on MI355X, the ladder of
    test_gpu_self_collision.py / the debug-and-production test: on the samples in which float64 iterates the kernel equals the f32 build in
    94.1 % / 96.3 % and is within one of it in 100 % / 99.5 %; the f32 and f32fma builds equal each other in 97.5 % / 95.3 % and are within
    one in 99.2 % / 99.0 %.

    Samples in which float64 does NOT iterate (no row carries force at qacc_smooth: 201 of 320 / 65 of 256) are a separate, exact matter.
    The kernel stops there too, in every one of them, on its gradient test (`solver_end`); the oracle's float32 builds never do: they run 1
    or 2 idle iterations in all of these samples.  On them they are no yardstick, and the kernel must simply do what float64 does.

    Asserted: (a) float64 does not iterate -> neither does the implementation, in every sample; (b) float64 iterates -> equal to the f32
    build's count in >= 90 % and within one of it in >= 98 % (of n samples at most ceil(0.02 n) further off; parity.py's Newton figures are 90 % and 99 %; the oracle's own two float32
    builds are within one of each other in 99.0 % here, which leaves an independent evaluation no margin at 99 %)."""
    got, f64, f32 = (np.asarray(x).astype(int) for x in (got, f64, f32))
    idle = f64 == 0
    assert (got[idle] == 0).all(), ("iterations where float64 makes none", np.nonzero(idle & (got != 0))[0][:10], got[idle & (got != 0)][:10])
    if (~idle).any():
        n, far = int((~idle).sum()), int((np.abs(got[~idle] - f32[~idle]) > 1).sum())
        eq = float((got[~idle] == f32[~idle]).mean())
        assert eq >= 0.90 and far <= np.ceil(0.02 * n), ("iteration count against the float32 oracle's, samples in which float64 iterates", n, eq, far)
        return eq, 1.0 - far / n
    return 1.0, 1.0


def assert_substep_criteria(out, impl, A, B):
    """`out` of parity.substep_ladder(impl, seq, A, B) with `impl` (the debug-dump instance), `A` (float64) and `B` (float32) wrapped in
    `Recording`.  C1 was judged inside the ladder from the kernel's own con_dist and limit distances; C3 and the limit rows as
    parity.assert_substep_criteria; C2 by assert_iteration_counts."""
    from tests import parity
    parity.check_quantiles(out["quantiles"], parity.SUBSTEP_FLOORS)
    assert out["limit_rows"]["lim_D"] < 1e-3 and out["limit_rows"]["lim_aref"] < 1e-3, out["limit_rows"]
    return assert_iteration_counts(impl.niter(), A.niter(), B.niter())


# ------------------------------------------------------------------------------------------ the debug dump of a candidate-pair model
def dyn_sections(d):
    """(name, size) of every section `rr_debug_layout` names for a candidate-pair model with dims `d`, in order.  The contact sections
    are per candidate pair; pen_count and slot_pair exist for these models only."""
    nb, nv, nM, nc = d.nbody, d.nv, d.nM, d.ncon
    return [("xpos", 3 * nb), ("xquat", 4 * nb), ("xmat", 9 * nb), ("subtree_com", 6), ("cinert", 10 * nb), ("crb", 10 * nb), ("cdof", 6 * nv),
            ("cvel", 6 * nb), ("cfrc", 6 * nb), ("qM", nM), ("qLD", nM), ("qLDiagInv", nv), ("qfrc_bias", nv), ("qfrc_passive", nv),
            ("qfrc_actuator", nv), ("qfrc_smooth", nv), ("qacc_smooth", nv), ("con_dist", nc), ("con_pos", 3 * nc), ("con_frame", 9 * nc),
            ("con_D", nc), ("con_aref", 4 * nc), ("limit_pos_D_aref", 3 * nv), ("qacc", nv), ("qfrc_constraint", nv), ("niter_cost", 2),
            ("ls_iters", 2), ("solver_end", 2), ("kernarg_ok", 1), ("pen_count", 1), ("slot_pair", SLOTS)]
