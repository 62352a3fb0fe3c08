"""The fixture of the domain-randomisation tests (test_randomisation_cpu.py, test_gpu_randomisation.py): G = 3 parameter sets

    geom_friction x {0.5, 1, 2}    dof_damping x {0.5, 1, 1.5}    dof_armature x {1, 2, 1}    actuator gain x {0.8, 1, 1.2}

(for a position-type actuator, biasprm[1] = -gain, the gain-coupled bias term is scaled by the same factor).  Set g as a model blob
is `with_parameters` + `save_blob`; env e of a mixed batch is on set e % 3.  Products are formed in float32, the precision the blob
stores, so that the blob of set g and row e of the batched tables hold the same cells."""
import os

import numpy as np

from rodent_amd import assets, mjcf

G = 3
FACTORS = dict(geom_friction=(0.5, 1.0, 2.0), dof_damping=(0.5, 1.0, 1.5), dof_armature=(1.0, 2.0, 1.0), gain=(0.8, 1.0, 1.2))


def base_fields(m):
    """The five supported fields of the model itself, shaped like MuJoCo's (gainprm / biasprm: the columns the blob stores)."""
    return dict(geom_friction=np.asarray(m["geom_friction"], np.float32), dof_damping=np.asarray(m["dof_damping"], np.float32),
                dof_armature=np.asarray(m["dof_armature"], np.float32), actuator_gainprm=np.asarray(m["actuator_gainprm0"], np.float32)[:, None],
                actuator_biasprm=np.asarray(m["actuator_biasprm"], np.float32))


def set_fields(m, g):
    """The fields of parameter set g."""
    f = base_fields(m)
    s = lambda k: np.float32(FACTORS[k][g])
    position = (f["actuator_biasprm"][:, 1] == -f["actuator_gainprm"][:, 0]) & (f["actuator_gainprm"][:, 0] != 0)
    bias = f["actuator_biasprm"].copy()
    bias[position, 1] = bias[position, 1] * s("gain")
    return dict(geom_friction=f["geom_friction"] * s("geom_friction"), dof_damping=f["dof_damping"] * s("dof_damping"),
                dof_armature=f["dof_armature"] * s("dof_armature"), actuator_gainprm=f["actuator_gainprm"] * s("gain"), actuator_biasprm=bias)


def mixed_fields(m, n):
    """[n, ...] fields: env e on set e % G."""
    sets = [set_fields(m, g) for g in range(G)]
    return {k: np.stack([sets[e % G][k] for e in range(n)]) for k in sets[0]}


def write_blobs(model_name, folder):
    """The G sets of `model_name` as blobs in `folder`; returns their paths WITHOUT the .rrm extension (what OracleEnvImpl /
    assets.asset_path take as a model name; `Rodent(xml_path=stem + '.rrm')` loads the blob as is)."""
    m = mjcf.load_blob(assets.asset_path(model_name))
    stems = []
    for g in range(G):
        stem = os.path.join(str(folder), f"{model_name}_set{g}")
        mjcf.save_blob(mjcf.with_parameters(m, **set_fields(m, g)), stem + ".rrm")
        stems.append(stem)
    return stems


def system_fn(fields_of):
    """A `randomization_fn(sys)` that puts `fields_of(sys.tables, num_envs)` ([N, ...] arrays of the blob's column counts) into `sys`."""
    def fn(sys, n):
        f = fields_of(sys.tables, n)
        gain = np.repeat(sys.actuator_gainprm[None], n, axis=0)
        bias = np.repeat(sys.actuator_biasprm[None], n, axis=0)
        gain[:, :, :1] = f["actuator_gainprm"]
        bias[:, :, :3] = f["actuator_biasprm"]
        new = sys.tree_replace(dict(geom_friction=f["geom_friction"], dof_damping=f["dof_damping"], dof_armature=f["dof_armature"],
                                    actuator_gainprm=gain, actuator_biasprm=bias))
        return new, {k: 0 for k in ("geom_friction", "dof_damping", "dof_armature", "actuator_gainprm", "actuator_biasprm")}
    return fn
