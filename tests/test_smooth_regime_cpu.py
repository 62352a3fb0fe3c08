"""The smooth regime on the CPU oracle alone (tests/smooth_regime.py; DESIGN.md section 2, "Per-entry parity"): the free variants'
tables, the regime facts on every shipped model, and the criterion itself -- it must accept a second, differently rounded float32
evaluation of the oracle on every field the GPU tests use, and reject a 5 % error in ONE distal parameter ten times over."""
import functools

import numpy as np
import pytest

from rodent_amd import assets, mjcf
from tests import randomisation_sets as rs, smooth_regime as sr, util

N = sr.N
ONE_SUBSTEP_FIELDS = sr.STAGE_FIELDS + sr.STEP_FIELDS[1:]


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_built):
    return oracle_built


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return tmp_path_factory.mktemp("smooth")


def _shipped(model):
    return mjcf.load_blob(assets.asset_path(model))


# ------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("model", sr.MODELS)
def test_rebuild_reproduces_the_shipped_tables(model):
    """The compiler's own functions on the raw fields of the blob, level schedules included: every derived table bit for bit (k_con_f
    apart: its effective-invweight cell needs the compiler's float64 inputs, and it reads no joint range)."""
    m = _shipped(model)
    got = sr.rebuild_tables(m)
    derived = [k for k in m if (k.startswith("k_") or k.startswith("h_")) and k not in sr.KEPT_TABLES]
    assert sorted(got) == sorted(derived)
    assert ("h_k_dof_f" in got) == (model == "rodent_pair")
    for k in derived:
        assert got[k].dtype == m[k].dtype and got[k].shape == m[k].shape and np.array_equal(got[k], m[k]), k


@pytest.mark.parametrize("model", sr.MODELS)
def test_free_variant_changes_the_range_cells_only(model):
    m = _shipped(model)
    f = sr.free_variant(m)
    assert sorted(f) == sorted(m)
    lim = m["jnt_limited"].astype(bool)
    assert lim.sum() == int(m["nlimit"]) >= 67
    assert np.array_equal(f["jnt_range"][lim], m["jnt_range"][lim] + np.float32([-sr.WIDEN, sr.WIDEN])) and np.array_equal(f["jnt_range"][~lim], m["jnt_range"][~lim])
    changed = {"jnt_range", "k_dof_f"} | ({"h_k_dof_f"} & set(m))
    for k in m:
        if k not in changed:
            assert f[k].dtype == m[k].dtype and np.array_equal(f[k], m[k]), k
    for pre in ("", "h_"):              # h_*: the tables of ONE replica of rodent_pair; its joints are the model's first ones
        if pre + "k_dof_f" not in m:
            continue
        kd, kd0, ki = f[pre + "k_dof_f"], m[pre + "k_dof_f"], f[pre + "k_dof_i"]
        jid, jr = ki[:, 1], f["jnt_range"]
        limited = ki[:, 8] == 1
        assert limited.sum() == (int(m["nlimit"]) if not pre else int(m["nlimit"]) // 2)
        assert np.array_equal(kd[limited][:, 4:6], jr[jid[limited]])                                # the kernel's cells ARE the raw field
        assert np.array_equal(kd[limited][:, 4:6], kd0[limited][:, 4:6] + np.float32([-sr.WIDEN, sr.WIDEN]))
        rest = np.ones(kd.shape, bool)
        rest[np.ix_(limited, [4, 5])] = False
        assert np.array_equal(kd[rest], kd0[rest])


# ------------------------------------------------------------------------------------------ regime facts, acceptance
@functools.lru_cache(maxsize=None)
def _case(folder, model, n_frames):
    """(free tables, inputs, float64 result with the regime facts asserted, f32 result, f32fma result), computed once."""
    stem = sr.free_blob(model, folder)
    st, ctrl, draws = sr.smooth_states(model, seed=0)
    want = sr.Oracle(stem, N, "f64").regime_facts(st, ctrl, n_frames)
    return mjcf.load_blob(stem + ".rrm"), (st, ctrl, draws), want, sr.Oracle(stem, N, "f32").step(st, ctrl, n_frames), sr.Oracle(stem, N, "f32fma").step(st, ctrl, n_frames)


def _accept_both_ways(fields, want, a, b, tab, what):
    for cand, yard, name in ((b, a, "f32fma by f32"), (a, b, "f32 by f32fma")):
        rec, bad = sr.judge(fields, cand, want, [yard], tab)
        print(what, name, {f: "%.2e <= %.2e" % (rec[f]["R"], rec[f]["bound"]) for f in fields})
        assert not bad, (what, name, {f: rec[f] for f in bad})


@pytest.mark.parametrize("model,n_frames", [(m, 1) for m in sr.MODELS] + [(m, 10) for m in sr.FLOOR_MODELS])
def test_regime_facts_and_acceptance_of_a_float32_evaluation(folder, model, n_frames):
    """The facts on the float64 oracle (asserted inside `_case`), the rodent_cpu sampler inside its cap, and each float32 build accepted
    with the other alone as yardstick on every field of the one-substep and ten-substep GPU cases -- with the plain entry scale
    (qM: sqrt(S_ii S_jj)), no field left out."""
    tab, (st, ctrl, draws), want, a, b = _case(folder, model, n_frames)
    assert st["qpos"].shape == (N, int(tab["nq"])) and np.abs(st["qvel"]).max() > 4.9
    assert N <= draws <= sr.MAX_DRAWS_PER_POSE * N and (draws > N) == (model == "rodent_cpu")
    print(model, n_frames, "draws", draws, "smallest con_dist", want["min_con_dist"])
    _accept_both_ways(ONE_SUBSTEP_FIELDS, want, a, b, tab, (model, n_frames))


def test_newton_and_parameter_sets(folder):
    """The two other one-substep cases of the GPU file: the Newton solver, and the batch whose env e runs on parameter set e % 3."""
    stem = sr.free_blob("rodent_optimized", folder)
    tab = mjcf.load_blob(stem + ".rrm")
    st, ctrl, _ = sr.smooth_states("rodent_optimized", seed=3)
    kw = dict(iterations=(4, 8), solver="newton")
    want = sr.Oracle(stem, N, "f64", **kw).regime_facts(st, ctrl)
    _accept_both_ways(sr.STEP_FIELDS, want, sr.Oracle(stem, N, "f32", **kw).step(st, ctrl), sr.Oracle(stem, N, "f32fma", **kw).step(st, ctrl), tab, "newton")
    stems = rs.write_blobs(stem, folder)
    sets = [mjcf.load_blob(s + ".rrm") for s in stems]
    assert all(np.array_equal(s["k_dof_f"][:, 4:6], tab["k_dof_f"][:, 4:6]) for s in sets)          # the sets keep the widened ranges
    assert not np.array_equal(sets[0]["k_dof_f"], sets[2]["k_dof_f"])
    want = sr.GroupedOracle(stems, N, "f64").regime_facts(st, ctrl)
    _accept_both_ways(sr.STEP_FIELDS, want, sr.GroupedOracle(stems, N, "f32").step(st, ctrl), sr.GroupedOracle(stems, N, "f32fma").step(st, ctrl), tab, "sets")


@pytest.mark.parametrize("steps,vz,seed", sr.ENV_CASES)
def test_env_forms(folder, steps, vz, seed):
    """The env-level cases (z = 0.4): facts, done == 0 on every step, acceptance on qpos, qvel and the observation segments."""
    stem = sr.free_blob("rodent_optimized", folder)
    tab = mjcf.load_blob(stem + ".rrm")
    st, actions, cur_frame = sr.env_inputs("rodent_optimized", steps, vz, seed)
    track = util.synthetic_track()
    want = sr.OracleEnv(stem, N, "f64", track).regime_facts(st, actions, cur_frame)
    assert 0.03 < want["qpos"][:, 2].min() and want["qpos"][:, 2].max() < 0.5
    a, b = (sr.OracleEnv(stem, N, p, track).steps(st, actions, cur_frame) for p in ("f32", "f32fma"))
    assert (a["done"] == 0).all() and np.array_equal(a["cur_frame"], want["cur_frame"])
    _accept_both_ways(sr.OBS_FIELDS, *(sr.obs_fields(x, tab) for x in (want, a, b)), tab, ("env", steps))


# ------------------------------------------------------------------------------------------ rejection
def _distal(tab, values):
    """Among the dofs with a non-zero value, a leaf of the dof tree where there is one, the deepest (the last of them)."""
    nv = int(tab["nv"])
    leaf = tab["k_dof_i"][:, 10] == np.arange(nv)
    c = np.nonzero((values != 0) & (leaf if (leaf & (values != 0)).any() else True))[0]
    return int(c[np.argmax(tab["dof_depth"][c] * 1000 + c)])


def _edits(tab):
    """name -> (raw field, index): the one cell that is made 5 % too large."""
    jointed = np.where(tab["body_jntnum"] > 0, tab["body_mass"], np.inf)
    jid = tab["dof_jntid"]
    u = int(np.argmax(tab["dof_depth"][tab["actuator_dofadr"]] * 1000 + np.arange(int(tab["nu"]))))
    return dict(mass=("body_mass", int(jointed.argmin())), damping=("dof_damping", _distal(tab, tab["dof_damping"])),
                armature=("dof_armature", _distal(tab, tab["dof_armature"])), gain=("actuator_gainprm0", u),
                stiffness=("jnt_stiffness", int(jid[_distal(tab, tab["jnt_stiffness"][jid])])))


def _edited(folder, tab, name):
    field, i = _edits(tab)[name]
    e = dict(tab)
    v = np.array(tab[field], copy=True)
    assert v[i] != 0
    v[i] *= np.float32(1.05)
    e[field] = v
    return sr.write_blob(e, folder, "edit_" + name)


@pytest.mark.parametrize("edit", ["mass", "damping", "armature", "gain", "stiffness"])
def test_seeded_error_is_rejected_ten_times_over(folder, edit):
    """The float32 oracle on a blob with one distal parameter 5 % off (the raw field: what the oracle reads), against the float64
    oracle on the free variant, both float32 builds as yardstick: at least one field exceeds its bound by 10x or more."""
    tab, (st, ctrl, _), want, a, b = _case(folder, "rodent_optimized", 1)
    ed = _edits(tab)
    assert ed["mass"][1] == 45 and tab["dof_depth"][ed["damping"][1]] == tab["dof_depth"].max()          # distal: the lightest body, the deepest leaf
    got = sr.Oracle(_edited(folder, tab, edit), N, "f32").step(st, ctrl)
    rec, bad = sr.judge(ONE_SUBSTEP_FIELDS, got, want, [a, b], tab)
    over = {f: rec[f]["R"] / rec[f]["bound"] for f in bad}
    print(edit, ed[edit], {f: "%.0fx" % v for f, v in over.items()})
    assert over and max(over.values()) >= 10.0, over
    assert max(over[f] for f in over if f in sr.STEP_FIELDS) > 1.0          # the production instances (no dump) see it too


def test_mass_edit_passes_the_global_scale_bounds(folder):
    """Why this criterion exists: the same 5 % mass error measured as the older tests measure -- largest error of a field over the
    largest magnitude of the field -- is inside their bounds (test_gpu_parity.py: qM 1e-6, qacc 4e-4, qvel 5e-3 of a global scale)."""
    tab, (st, ctrl, _), want, a, b = _case(folder, "rodent_optimized", 1)
    got = sr.Oracle(_edited(folder, tab, "mass"), N, "f32").step(st, ctrl)
    glob = lambda f: float(np.abs(got[f] - want[f]).max() / np.abs(want[f]).max())
    dv = np.abs(want["qvel"] - st["qvel"]).max(1)
    qvel = float((np.abs(got["qvel"] - want["qvel"]).max(1) / np.maximum(dv, 1e-3)).max())           # test_solver_and_substep_match_oracle's scale
    rec, _ = sr.judge(("qM", "qfrc_bias", "qacc"), got, want, [a, b], tab)
    print("mass of body 45 x 1.05, global-max figures against the suite's bounds: qM %.2e (1e-6)  qfrc_bias %.2e (3e-6)  qacc %.2e (4e-4)  qvel %.2e (5e-3)"
          % (glob("qM"), glob("qfrc_bias"), glob("qacc"), qvel))
    print("per entry: " + "  ".join("%s %.2e (bound %.2e)" % (f, rec[f]["R"], rec[f]["bound"]) for f in rec))
    assert glob("qM") < 1e-6 and glob("qacc") < 4e-4 and qvel < 5e-3
    assert all(rec[f]["R"] > 10 * rec[f]["bound"] for f in rec)
