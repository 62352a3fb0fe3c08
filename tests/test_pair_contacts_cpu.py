"""The per-pair contact criterion and its cases (tests/pair_contact_cases.py) on the CPU oracle alone: each case is in the regime it
claims, the conditioning filter leaves out at most 1 % of a kind's pair-samples, the oracle's two float32 builds pass the criterion
against each other, and three seeded errors do not."""
import numpy as np
import pytest

from rodent_amd import assets, hip
from tests import pair_contact_cases as pc
from tests import smooth_regime as sr

CASES = ("shipped", "dense", "spheres", "overflow")
GEOMETRY_CASES = ("shipped", "dense", "spheres")


@pytest.fixture(scope="module")
def cases(oracle_built, tmp_path_factory):
    """case -> dict(m, stem, st, ctrl, A, want, keep, ys): blob, inputs, the float64 forward pass, the kept samples, the float32 builds."""
    folder = tmp_path_factory.mktemp("pair_blobs")
    out = {}
    for case in CASES:
        m, stem = pc.variant(case), pc.blob(case, folder)
        st, ctrl = pc.inputs(case, stem)
        A = pc.PairOracle(stem, pc.N, "f64").forward(st, ctrl)
        cond = pc.conditioning(m, A.get("geom_xpos").reshape(pc.N, -1, 3), A.get("geom_xmat"))
        ys = [pc.PairOracle(stem, pc.N, p).forward(st, ctrl).geometry() for p in ("f32", "f32fma")]
        out[case] = dict(m=m, stem=stem, st=st, ctrl=ctrl, A=A, want=A.geometry(), cond=cond, keep=pc.kept_samples(cond), ys=ys, folder=folder)
    return out


def test_regime_facts(cases):
    m0 = pc.shipped()
    kind, dims = np.asarray(m0["con_kind"]), np.asarray(m0["con_dim"])
    assert [int((kind == k).sum()) for k in pc.KINDS] == [18, 811, 1414]
    for case, c in cases.items():
        dist = c["want"]["dist"]
        pen = dist < 0
        print(case, "pairs in penetration per env: mean %.1f max %d | by kind %s | by condim %s" %
              (pen.sum(1).mean(), pen.sum(1).max(), [int(pen[:, kind == k].sum()) for k in pc.KINDS], [int(pen[:, dims == k].sum()) for k in (1, 3)]))
        pc.assert_regime(case, dist)


def test_filter_reads_the_oracles_own_geometry_and_stays_within_the_cap(cases):
    for case in GEOMETRY_CASES:
        c = cases[case]
        assert np.abs(c["cond"]["dist"] - c["want"]["dist"]).max() < 1e-13      # the numpy restatement IS the oracle's pair geometry
        shares = pc.excluded_shares(c["m"], c["keep"])
        print(case, {k: "%.4f" % v for k, v in shares.items() if v > 0})
        assert max(shares.values()) <= pc.MAX_EXCLUDED, shares
        assert all(v == 0 for (k, f), v in shares.items() if f == "dist")


@pytest.mark.parametrize("case", GEOMETRY_CASES)
def test_float32_builds_pass_against_each_other(cases, case):
    c = cases[case]
    for i in (0, 1):
        rec, bad = pc.judge(c["m"], c["ys"][i], c["want"], [c["ys"][1 - i]], c["keep"])
        print(case, ("f32", "f32fma")[i], "as the implementation\n" + pc.report({k: dict(v, yard=v["yard"] * 2) for k, v in rec.items()}))
        assert not bad, bad


def _most_used(m, kinds, gtype):
    """The geom of type `gtype` that occurs in the most candidate pairs of `kinds`."""
    from rodent_amd import mjcf
    sel = np.isin(np.asarray(m["con_kind"]), kinds)
    g = np.concatenate([np.asarray(m["con_geom1"])[sel], np.asarray(m["con_geom2"])[sel]])
    g = g[np.asarray(m["geom_type"])[g] == getattr(mjcf, gtype)]
    return int(np.bincount(g).argmax())


def test_seeded_errors_are_rejected(cases):
    c = cases["dense"]
    m = c["m"]
    # a capsule's half length off by 1 %
    cap = _most_used(m, (6,), "CAPSULE")
    e1 = dict(m)
    e1["geom_size"] = np.array(m["geom_size"], copy=True)
    e1["geom_size"][cap, 1] *= np.float32(1.01)
    # a sphere's local position off by 1e-4 m
    sph = _most_used(m, (4, 5), "SPHERE")
    e2 = dict(m)
    e2["geom_pos"] = np.array(m["geom_pos"], copy=True)
    e2["geom_pos"][sph, 0] += np.float32(1e-4)
    for name, em in (("half_length", e1), ("sphere_pos", e2)):
        stem = sr.write_blob(pc.retabled(em), c["folder"], "rodent_cpu_" + name)
        got = pc.PairOracle(stem, pc.N, "f32").forward(c["st"], c["ctrl"]).geometry()
        rec, bad = pc.judge(m, got, c["want"], c["ys"], c["keep"])
        print(name, bad)
        assert any("dist" in b or "pos" in b for b in bad), (name, bad)
    # one pair-sample's normal negated in an otherwise passing result
    kind = np.asarray(m["con_kind"])
    for k in pc.KINDS:
        env, pair = np.argwhere(c["keep"]["normal"] & (kind == k)[None])[7]
        got = {f: v.copy() for f, v in c["ys"][0].items()}
        got["frame"][env, pair, :3] *= -1
        rec, bad = pc.judge(m, got, c["want"], c["ys"], c["keep"])
        assert len(bad) == 1 and bad[0].startswith(f"kind {k} normal"), bad


def test_variant_tables_carry_the_edited_sizes(cases):
    m0 = pc.shipped()
    g1, g2 = np.asarray(m0["con_geom1"]), np.asarray(m0["con_geom2"])
    for case in ("dense", "spheres", "overflow"):
        m = cases[case]["m"]
        kf, kf0 = np.asarray(m["k_con_f"]).reshape(-1, 32), np.asarray(m0["k_con_f"]).reshape(-1, 32)
        size = np.asarray(m["geom_size"], np.float32)
        assert np.array_equal(kf[:, 7:10], size[g1]) and np.array_equal(kf[:, 17:20], size[g2])
        assert not np.array_equal(kf[:, 7], kf0[:, 7])                                  # the edit did arrive
        assert np.array_equal(size[:, 1:], np.asarray(m0["geom_size"], np.float32)[:, 1:])
        rest = [c for c in range(32) if c not in (7, 17, 21)]
        assert np.array_equal(kf[:, rest], kf0[:, rest])
        # cell 21, the effective invweight: formed from the blob's float32 fields here, from float64 ones in the shipped table (sr.KEPT_TABLES)
        assert np.abs(kf[:, 21] - kf0[:, 21]).max() <= 2.0 ** -22 * np.abs(kf0[:, 21]).max()
        for k in m0:
            if k not in ("geom_size", "k_con_f"):
                assert np.array_equal(np.asarray(m[k]), np.asarray(m0[k])), (case, k)
    f = pc.SPHERES_FACTOR
    sp = pc.sphere_pair_geoms(m0)
    s0, s1 = np.asarray(m0["geom_size"], np.float64), np.asarray(cases["spheres"]["m"]["geom_size"], np.float64)
    assert np.allclose(s1[sp, 0], f * s0[sp, 0], rtol=1e-6) and np.array_equal(np.delete(s1, sp, 0), np.delete(s0, sp, 0))


def test_debug_layout_of_a_candidate_pair_model():
    """The dump of a candidate-pair model: the shared sections with the contact ones per pair, then pen_count and slot_pair; the
    floor-contact models' dump ends at kernarg_ok as before."""
    d = hip.Model(assets.asset_path("rodent_cpu")).dims
    sec = pc.dyn_sections(d)
    assert d.dbg_floats == sum(n for _, n in sec) and sec[-2:] == [("pen_count", 1), ("slot_pair", 64)]
    f = hip.Model(assets.asset_path("rodent_0")).dims
    assert f.dbg_floats == sum(n for _, n in pc.dyn_sections(f)[:-2])
