"""Domain randomisation without a GPU: the per-env kernel rows (`ktables.env_param_tables`) against the blobs `with_parameters` builds,
the refusals of unsupported / mis-shaped fields, `System.replace`, and the code-object metadata of the rr_rand_kernel instances.
Fixture: tests/randomisation_sets.py (three parameter sets on rodent_optimized and rodent_new)."""
import ctypes
import os
import sys

import numpy as np
import pytest

from rodent_amd import assets, hip, mjcf
from rodent_amd.ktables import ENV_PARAM_FIELDS, env_param_tables, with_parameters
from tests import randomisation_sets as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ("rodent_optimized", "rodent_new")


@pytest.mark.parametrize("name", MODELS)
def test_env_rows_equal_the_rows_of_the_set_blobs(name, tmp_path):
    m = mjcf.load_blob(assets.asset_path(name))
    N = 8
    dof_f, act_f, con_f = env_param_tables(m, rs.mixed_fields(m, N))
    assert dof_f.shape == (N, int(m["nv"]), 16) and act_f.shape == (N, int(m["nu"]), 8) and con_f.shape == (N, int(m["ncon"]), 26)
    assert dof_f.dtype == act_f.dtype == con_f.dtype == np.float32
    blobs = [mjcf.load_blob(stem + ".rrm") for stem in rs.write_blobs(name, tmp_path)]      # through save_blob: what the oracle and the env load
    for e in range(N):
        b = blobs[e % rs.G]
        assert np.array_equal(dof_f[e], b["k_dof_f"]) and np.array_equal(act_f[e], b["k_act_f"]) and np.array_equal(con_f[e], b["k_con_f"]), e
    # the sets do differ, in the cells they should: armature (0) / damping (1); gain (0) and the position actuators' bias (2); mu (16) / invweight (17)
    assert np.array_equal(np.nonzero((dof_f[0] != dof_f[1]).any(0))[0], [0, 1])
    assert set(np.nonzero((act_f[0] != act_f[2]).any(0))[0]) <= {0, 2} and (act_f[0][:, 0] != act_f[2][:, 0]).any()
    assert np.array_equal(np.nonzero((con_f[0] != con_f[2]).any(0))[0], [16, 17])
    # ... and the MuJoCo-named fields the oracle reads follow
    assert np.array_equal(blobs[0]["con_friction"][:, 0], blobs[0]["k_con_f"][:, 16])
    assert np.array_equal(blobs[2]["dof_damping"], m["dof_damping"] * np.float32(1.5))
    assert np.array_equal(blobs[1]["dof_armature"], m["dof_armature"] * np.float32(2.0))
    assert np.array_equal(blobs[2]["actuator_gainprm0"], m["actuator_gainprm0"] * np.float32(1.2))
    for k in ("dof_invweight0", "con_invweight", "body_invweight0", "stat_meaninertia", "k_dof_i", "k_con_i", "k_body_f"):     # stay as compiled
        assert np.array_equal(blobs[0][k], m[k]), k


def test_con_friction_follows_the_mixing_rule():
    """Equal priorities: the max over the pair; otherwise the geom of higher priority decides (mjcf._collision_tables)."""
    m = mjcf.load_blob(assets.asset_path("rodent_optimized"))
    g1, g2 = m["con_geom1"], m["con_geom2"]
    p1, p2 = m["geom_priority"][g1], m["geom_priority"][g2]
    f = m["geom_friction"].copy()
    f[g2[0]] = f[g2[0]] * np.float32(0.25)
    f[g2[-1]] = f[g2[-1]] * np.float32(4.0)
    f[g1[0]] = f[g1[0]] * np.float32(3.0)              # the floor
    b = with_parameters(m, geom_friction=f)
    want = np.where((p1 == p2)[:, None], np.maximum(f[g1], f[g2]), np.where((p1 > p2)[:, None], f[g1], f[g2]))
    assert np.array_equal(b["con_friction"], np.stack([want[:, 0], want[:, 0], want[:, 1], want[:, 2], want[:, 2]], 1))
    assert np.array_equal(b["k_con_f"][:, 16], want[:, 0])
    mu, ciw = want[:, 0].astype(np.float64), m["con_invweight"].astype(np.float64)
    invw = ((ciw + mu * mu * ciw) * 2 * mu * mu / float(m["opt_impratio"])).astype(np.float32)
    changed = want[:, 0] != m["k_con_f"][:, 16]
    assert changed.any() and not changed.all() and np.array_equal(b["k_con_f"][changed, 17], invw[changed])
    assert np.array_equal(b["k_con_f"][~changed, 17], m["k_con_f"][~changed, 17])
    # an equal-priority pair: a synthetic two-contact view of the same model
    m2 = dict(m, geom_priority=np.zeros_like(m["geom_priority"]))
    b2 = with_parameters(m2, geom_friction=f)
    assert np.array_equal(b2["con_friction"][:, 0], np.maximum(f[g1], f[g2])[:, 0])


@pytest.mark.parametrize("name", MODELS + ("rodent_0",))
def test_identity_draw_reproduces_the_shipped_rows(name):
    m = mjcf.load_blob(assets.asset_path(name))
    N = 5
    ident = {k: np.repeat(v[None], N, axis=0) for k, v in rs.base_fields(m).items()}
    dof_f, act_f, con_f = env_param_tables(m, ident)
    for e in range(N):
        assert np.array_equal(dof_f[e], m["k_dof_f"]) and np.array_equal(act_f[e], m["k_act_f"]) and np.array_equal(con_f[e], m["k_con_f"])
    same = with_parameters(m, **rs.base_fields(m))
    assert set(same) == set(m)
    for k in m:
        assert np.array_equal(same[k], m[k]) and same[k].dtype == m[k].dtype, k
    # MuJoCo's ten columns are taken as well (the first 1 / 3 are used)
    pad = lambda a: np.concatenate([a, np.zeros((a.shape[0], 10 - a.shape[1]), np.float32)], axis=1)
    wide = with_parameters(m, actuator_gainprm=pad(rs.base_fields(m)["actuator_gainprm"]), actuator_biasprm=pad(rs.base_fields(m)["actuator_biasprm"]))
    assert np.array_equal(wide["k_act_f"], m["k_act_f"])


def test_unsupported_and_misshaped_fields_are_refused():
    m = mjcf.load_blob(assets.asset_path("rodent_optimized"))
    N, nv = 4, int(m["nv"])
    with pytest.raises(ValueError, match="body_mass") as ei:
        env_param_tables(m, dict(body_mass=np.ones((N, int(m["nbody"])), np.float32)))
    for k in ENV_PARAM_FIELDS:
        assert k in str(ei.value)
    with pytest.raises(ValueError, match="body_inertia"):
        with_parameters(m, body_inertia=m["body_inertia"])
    with pytest.raises(ValueError, match="dof_damping"):
        env_param_tables(m, dict(dof_damping=np.ones((N, nv + 1), np.float32)))
    with pytest.raises(ValueError, match="dof_armature"):
        env_param_tables(m, dict(dof_armature=np.ones(nv, np.float32)))                 # no env axis
    with pytest.raises(ValueError, match="geom_friction"):
        with_parameters(m, geom_friction=np.ones((int(m["ngeom"]), 2), np.float32))
    with pytest.raises(ValueError, match="actuator_biasprm"):
        with_parameters(m, actuator_biasprm=np.ones((int(m["nu"]), 2), np.float32))      # fewer than the three columns in use
    with pytest.raises(ValueError, match="disagree"):
        env_param_tables(m, dict(dof_damping=np.ones((N, nv), np.float32), dof_armature=np.ones((N + 1, nv), np.float32)))
    for name in ("rodent_cpu", "rodent_pair"):                                           # no kernel instance reads per-env rows for these
        with pytest.raises(ValueError, match="not supported"):
            with_parameters(mjcf.load_blob(assets.asset_path(name)), dof_damping=np.ones(1, np.float32))


def test_system_replace_leaves_the_original_alone():
    from rodent_amd.envs.base import System
    s = System(assets.asset_path("rodent_optimized"), 8, 8)
    assert s.geom_friction.shape == (101, 3) and s.dof_damping.shape == (73,) and s.dof_armature.shape == (73,)
    assert s.actuator_gainprm.shape == (30, 10) and s.actuator_biasprm.shape == (30, 10)
    assert np.array_equal(s.actuator_gainprm[:, 0], s.tables["actuator_gainprm0"]) and np.array_equal(s.actuator_biasprm[:, :3], s.tables["actuator_biasprm"])
    assert set(System.PARAM_FIELDS) == set(ENV_PARAM_FIELDS)
    before = {k: getattr(s, k).copy() for k in System.PARAM_FIELDS}
    fr = np.repeat(s.geom_friction[None], 4, axis=0) * np.float32(2)
    s2 = s.replace(geom_friction=fr)
    s3 = s.tree_replace({"dof_damping": s.dof_damping * np.float32(0.5), "geom_friction": fr})
    assert s2 is not s and s2.geom_friction is fr and s3.geom_friction is fr and s2.dof_damping is s.dof_damping
    assert np.array_equal(s3.dof_damping, before["dof_damping"] * np.float32(0.5))
    for k, v in before.items():
        assert np.array_equal(getattr(s, k), v), k
    assert s2.model is s.model and s2.nv == s.nv
    assert np.array_equal(s.body_mass, s.tables["body_mass"])             # any other table reads through
    with pytest.raises(AttributeError):
        s.replace(no_such_field=1)
    with pytest.raises(ValueError, match="nested"):
        s.tree_replace({"opt.timestep": 0.001})


def test_rank_key_split():
    from rodent_amd.training.agents.ppo.train import randomization_keys
    k0, e0 = randomization_keys(0, 0, 32, 16)
    k1, e1 = randomization_keys(0, 1, 32, 16)
    assert k0.shape == (32, 2) and e0.shape == (16, 2) and k0.dtype == np.uint32
    assert not np.array_equal(k0, k1) and not np.array_equal(e0, e1)
    assert len({tuple(k) for k in np.concatenate([k0, k1, e0, e1])}) == 96          # every env of both ranks has its own key
    assert np.array_equal(randomization_keys(0, 0, 32, 16)[0], k0)


def test_rand_kernel_instances_in_the_code_object():
    """Nine instances of the entry with per-env parameters (three dimension classes x single-step / multi-step / multi-step with the
    actor); each within the budget of the production instances (no scratch, no VGPR spill, two waves per SIMD), without static LDS, and
    with the I/O block where the host (`rr_kernarg_layout`) and the kernel's re-reads assume it -- the argument list of rr_step_kernel."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = [k for k in kernel_meta.kernels(hip.LIB_PATH) if "rr_rand_kernel" in k["name"]]
    assert len(ks) == 9, [k["name"] for k in ks]
    assert not any("rr_step_kernel" in k["name"] for k in ks)
    assert sum("RRDimsFixedILi66ELi59ELi1263EE" in k["name"] for k in ks) == 3 and sum("RRDimsFixedILi67ELi57ELi1279EE" in k["name"] for k in ks) == 3
    off, size, total = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    hip.lib().rr_kernarg_layout(ctypes.byref(off), ctypes.byref(size), ctypes.byref(total))
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["vgpr"] + k["agpr"] <= 256, k
        assert k["lds"] == 0, k
        explicit = [a for a in k["args"] if a[2] == "by_value"]
        assert len(explicit) == 5, k["name"]
        assert explicit[0][0] == 0 and explicit[1][1] == 22 * 8 and explicit[1][0] + explicit[1][1] == explicit[2][0]
        assert explicit[2][:2] == (off.value, size.value), (k["name"], explicit)
        assert explicit[4][0] + explicit[4][1] == total.value
