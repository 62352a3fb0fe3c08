"""`State` / `PipelineState` / `PipelineEnv`: the torch-tensor mirror of `brax.envs.base`
(the reference imports `PipelineEnv, State` from there [REF Rodent_Env_Brax.py:4]).

Batched by construction: every leaf has a leading env axis [N, ...] instead of being vmapped.
"""
from __future__ import annotations

import dataclasses
from typing import Any, Dict, Optional

import numpy as np
import torch

from .. import assets, hip


@dataclasses.dataclass
class PipelineState:
    """What the reference env reads from `mjx.Data` [REF Rodent_Env_Brax.py:110,116,151-155,161]."""
    qpos: torch.Tensor            # [N, nq]
    qvel: torch.Tensor            # [N, nv]
    act: torch.Tensor             # [N, na]
    qacc_warmstart: torch.Tensor  # [N, nv]
    # Derived quantities of the last forward pass.  `Rodent.step` leaves them None unless the env was built with
    # `pipeline_outputs=True`: the observation already carries cinert / cvel / qfrc_actuator [REF Rodent_Env_Brax.py:151-155]
    # and writing them a second time was 7.7 KB per env-step of HBM traffic (+ the AutoReset select over them).
    cinert: Optional[torch.Tensor] = None          # [N, nbody, 10]
    cvel: Optional[torch.Tensor] = None            # [N, nbody, 6]
    qfrc_actuator: Optional[torch.Tensor] = None   # [N, nv]
    xpos: Optional[torch.Tensor] = None            # [N, nbody, 3]
    xmat: Optional[torch.Tensor] = None            # [N, nbody, 9]
    # brax `State.contact` (mjx.Data.contact) geometry [NB mjcf.ipynb:917-921]; filled with `contact_outputs=True`;
    # the static integer fields are `sys.contact_geom1 / contact_geom2 / contact_link_idx`
    contact_dist: Optional[torch.Tensor] = None    # [N, ncon]
    contact_pos: Optional[torch.Tensor] = None     # [N, ncon, 3]
    contact_frame: Optional[torch.Tensor] = None   # [N, ncon, 3, 3]

    @property
    def q(self):
        return self.qpos

    @property
    def qd(self):
        return self.qvel

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)

    def tree(self):
        return {f.name: getattr(self, f.name) for f in dataclasses.fields(self) if getattr(self, f.name) is not None}


@dataclasses.dataclass
class Contact:
    """brax `State.contact` / `mjx.Data.contact` with the fields the reference's notebook shows [NB mjcf.ipynb:917-921]:
    per-step geometry from the kernel (`contact_outputs=True`), static parameters and integer ids from the loaded model
    (C ABI `rr_model_table`).  Leading env axis on the per-step fields."""
    dist: torch.Tensor            # [N, ncon]
    pos: torch.Tensor             # [N, ncon, 3]
    frame: torch.Tensor           # [N, ncon, 3, 3]
    includemargin: torch.Tensor   # [ncon] (0: the rodent models use no margin)
    friction: torch.Tensor        # [ncon, 5]
    solref: torch.Tensor          # [ncon, 2]
    solreffriction: torch.Tensor  # [ncon, 2] (0)
    solimp: torch.Tensor          # [ncon, 5]
    geom1: torch.Tensor           # [ncon] int32
    geom2: torch.Tensor           # [ncon] int32
    link_idx: tuple               # (geom_bodyid[geom1] - 1, geom_bodyid[geom2] - 1), int32 [ncon] each
    elasticity: torch.Tensor      # [ncon] (0)


@dataclasses.dataclass
class State:
    """Environment state for training and inference (brax.envs.base.State)."""
    pipeline_state: Optional[PipelineState]
    obs: torch.Tensor
    reward: torch.Tensor
    done: torch.Tensor
    metrics: Dict[str, torch.Tensor] = dataclasses.field(default_factory=dict)
    info: Dict[str, Any] = dataclasses.field(default_factory=dict)

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


class System:
    """The few `sys.*` attributes the reference env touches [REF Rodent_Env_Brax.py:82-89], and the model parameters a
    `randomization_fn` may replace (brax: `sys.tree_replace({'geom_friction': ...})`): numpy arrays under MuJoCo's names,
    `geom_friction` [ngeom, 3], `dof_damping` [nv], `dof_armature` [nv], `actuator_gainprm` [nu, 10] (column 0: the gain),
    `actuator_biasprm` [nu, 10] (columns 0..2).  Any other table of the blob reads as `sys.<name>` too."""

    PARAM_FIELDS = ("geom_friction", "dof_damping", "dof_armature", "actuator_gainprm", "actuator_biasprm")

    def __init__(self, blob_path: str, iterations: int, ls_iterations: int, solver: str = "cg"):
        from .. import mjcf
        self.blob_path = blob_path
        self.tables = mjcf.load_blob(blob_path)
        self.model = hip.Model(blob_path, iterations=iterations, ls_iterations=ls_iterations, solver=solver)
        self.solver = solver.lower()
        d = self.model.dims
        self.nq, self.nv, self.nu, self.na, self.nbody = d.nq, d.nv, d.nu, d.na, d.nbody
        self.obs_dim = d.obs_dim
        self.dt = float(d.timestep)
        self.qpos0 = self.tables["qpos0"]
        self.ncon = d.ncon
        # the contact list is a list of CANDIDATE pairs of two moving geoms (rodent_cpu.xml): pairs in penetration beyond the kernel's
        # contact slots are dropped and counted (`Rodent.contact_overflow`)
        self.candidate_contacts = bool(int(np.asarray(self.tables.get("k_dyn", 0)).reshape(-1)[0]))
        # integer ids as the LOADED model holds them (C ABI rr_model_table): Contact.geom1 / geom2 and brax's link_idx
        # (= geom_bodyid[g] - 1) [NB mjcf.ipynb:917-921]
        self.contact_geom1 = self.model.table("con_geom1")
        self.contact_geom2 = self.model.table("con_geom2")
        self.geom_bodyid = self.model.table("geom_bodyid")
        self.contact_link_idx = (self.geom_bodyid[self.contact_geom1] - 1, self.geom_bodyid[self.contact_geom2] - 1)
        t = self.tables
        self.geom_friction = t["geom_friction"].copy()
        self.dof_damping = t["dof_damping"].copy()
        self.dof_armature = t["dof_armature"].copy()
        self.actuator_gainprm = np.zeros((self.nu, 10), np.float32)
        self.actuator_gainprm[:, 0] = t["actuator_gainprm0"]
        self.actuator_biasprm = np.zeros((self.nu, 10), np.float32)
        self.actuator_biasprm[:, :3] = t["actuator_biasprm"]

    def __getattr__(self, name):           # (only reached for names not set above) any other table of the blob, read-only use
        tables = self.__dict__.get("tables")
        if tables is not None and name in tables:
            return tables[name]
        raise AttributeError(name)

    def replace(self, **kw) -> "System":
        """A copy with the given attributes replaced (brax `sys.replace`); the original is left as it is."""
        import copy
        new = copy.copy(self)
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(f"System has no field '{k}'")
            setattr(new, k, v)
        return new

    def tree_replace(self, params: Dict[str, Any]) -> "System":
        """brax `sys.tree_replace({'geom_friction': x, ...})`; nested (dotted) names are not part of this System."""
        for k in params:
            if "." in k:
                raise ValueError(f"System.tree_replace: nested field '{k}' is not supported")
        return self.replace(**params)


class PipelineEnv:
    """API for driving the HIP physics backend (`brax.envs.base.PipelineEnv` with backend='mjx'
    replaced by the fused HIP kernel): `pipeline_init` / `pipeline_step` [REF Rodent_Env_Brax.py:87,101]."""

    def __init__(self, sys: System, num_envs: int, n_frames: int = 1, backend: str = "hip", device=None, debug=False,
                 pipeline_outputs: bool = False, contact_outputs: bool = False, balance: Optional[bool] = None, rebalance_every: int = 4):
        if backend not in ("hip", "mjx"):
            raise ValueError(f"backend {backend!r} not available: this build provides the HIP backend only")
        self.sys = sys
        self._n_frames = n_frames
        self._debug = debug
        self._pipeline_outputs = pipeline_outputs
        self._contact_outputs = contact_outputs
        self.num_envs = int(num_envs)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._batch = hip.Batch(sys.model, self.num_envs, self.device)
        # SIMD pairing (scheduling only; results are unaffected; OFF by default).  When the batch is exactly one resident round of
        # the GPU (2 waves per SIMD: N = 8 x CUs), workgroups w and w + N/2 share a SIMD and the launch lasts as long as its
        # slowest environment.  With `balance=True` the envs are re-mapped every `rebalance_every` steps so that the costliest
        # ones of the last launch (work estimate reported by the kernel) sit with the cheapest ones.  With the TRUE cost of the
        # step being launched the effect is real (MI355X, same 2048 states: heavy|light pairs 1.412 ms, random 1.452 ms,
        # heavy|heavy 1.519 ms; tools/pairing_probe.py), but the previous step's cost does not predict it well enough under
        # random actions: the bench measured 1.5027 ms balanced against 1.5038 ms unbalanced, so it stays an option.
        self._balance = bool(balance)
        self._rebalance_every, self._launches = max(1, int(rebalance_every)), 0
        if self._balance:
            self._env_map = torch.arange(self.num_envs, dtype=torch.int32, device=self.device)
            self._cost = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
            self._batch.set_schedule(self._env_map, self._cost)

    # -- domain randomisation
    def randomize(self, randomization_fn):
        """Per-environment model parameters, as `brax.envs.wrappers.training.DomainRandomizationVmapWrapper` takes them:
        `randomization_fn(sys)` -- keys already bound, e.g. `functools.partial(fn, rng=keys[N, 2])` -- returns `(sys_v, in_axes)`, a
        System whose randomised fields carry a leading env axis [N, ...] and, per field, 0 (batched) or None; `in_axes` may be a dict
        {field: 0 | None}, an object with such attributes, or None (then the fields whose arrays gained a leading axis are the batched
        ones).  Supported fields: System.PARAM_FIELDS.  The kernel rows are rebuilt per env (`ktables.env_param_tables`) and uploaded;
        the parameters stay fixed per env until the next call (brax does not re-draw them at reset either)."""
        from .. import ktables
        if not self._batch.env_params_supported():
            self._batch.set_env_params(*(torch.zeros(self.num_envs, r, w, device=self.device) for r, w in
                                         ((self.sys.nv, 16), (self.sys.nu, 8), (self.sys.ncon, 26))))      # raises with the library's reason
        sys_v, in_axes = randomization_fn(self.sys)
        axis = (lambda k: None) if in_axes is None else ((lambda k: in_axes.get(k)) if isinstance(in_axes, dict) else (lambda k: getattr(in_axes, k, None)))
        names = set(System.PARAM_FIELDS) | (set(in_axes) if isinstance(in_axes, dict) else set())
        names |= {k for k, v in vars(sys_v).items() if isinstance(v, (np.ndarray, torch.Tensor)) and v is not getattr(self.sys, k, None)}
        batched = {}
        for k in sorted(names):
            new, old = getattr(sys_v, k, None), getattr(self.sys, k, None)
            if new is None or (new is old and axis(k) is None):
                continue
            new = new.detach().cpu().numpy() if torch.is_tensor(new) else np.asarray(new)
            is_b = axis(k) == 0 if in_axes is not None else (old is not None and new.ndim == np.ndim(old) + 1)
            if axis(k) not in (None, 0):
                raise ValueError(f"randomize: in_axes['{k}'] must be 0 or None")
            if not is_b:
                if old is not None and new.shape == np.shape(old) and np.array_equal(new, old):
                    continue
                if k not in System.PARAM_FIELDS or old is None or new.shape != np.shape(old):
                    raise ValueError(f"randomize: field '{k}' was replaced but is not marked batched with a leading env axis; the supported "
                                     f"fields are {', '.join(System.PARAM_FIELDS)}")
                new = np.broadcast_to(new, (self.num_envs,) + new.shape)     # one new value for all envs
            elif new.ndim < 1 or new.shape[0] != self.num_envs:
                raise ValueError(f"randomize: batched field '{k}' has shape {new.shape}, expected a leading axis of {self.num_envs} envs")
            batched[k] = new
        dof_f, act_f, con_f = ktables.env_param_tables(self.sys.tables, batched)
        up = lambda a: torch.from_numpy(a).to(self.device)
        self.set_env_params(dof_f=up(dof_f) if {"dof_damping", "dof_armature"} & set(batched) else None,
                            act_f=up(act_f) if {"actuator_gainprm", "actuator_biasprm"} & set(batched) else None,
                            con_f=up(con_f) if "geom_friction" in batched else None)
        return sys_v

    def set_env_params(self, dof_f=None, act_f=None, con_f=None):
        """Upload per-env kernel rows (float32 device tensors as `ktables.env_param_tables` builds them; None = the model's shared table;
        all None clears them)."""
        self._batch.set_env_params(dof_f, act_f, con_f)
        self._env_params = None if dof_f is None and act_f is None and con_f is None else dict(dof_f=dof_f, act_f=act_f, con_f=con_f)

    def env_params(self):
        """The per-env rows in force: {'dof_f', 'act_f', 'con_f'} (device tensors or None per table), or None without randomisation."""
        return getattr(self, "_env_params", None)

    def _rebalance(self):
        """Call before a step launch: every `rebalance_every` launches, pair heavy with light environments."""
        if not self._balance:
            return
        self._launches += 1
        if self._launches % self._rebalance_every == 0:
            order = torch.argsort(self._cost, descending=True)
            half = self.num_envs // 2
            self._env_map[:half] = order[:half]
            self._env_map[half:] = order.flip(0)[:half]

    # -- brax surface
    @property
    def dt(self) -> float:
        return self.sys.dt * self._n_frames

    @property
    def observation_size(self) -> int:
        return self.sys.obs_dim

    @property
    def action_size(self) -> int:
        return self.sys.nu

    @property
    def backend(self) -> str:
        return "hip"

    def _alloc_outputs(self, full: bool = True):
        """Buffers for the optional rr_outputs; `full=False` honours the env's pipeline_outputs / contact_outputs switches
        (the rollout path: nothing unless asked for)."""
        N, s, dev = self.num_envs, self.sys, self.device
        out = {}
        if full or self._pipeline_outputs:
            out.update(cinert=torch.empty(N, s.nbody, 10, device=dev), cvel=torch.empty(N, s.nbody, 6, device=dev),
                       qfrc_actuator=torch.empty(N, s.nv, device=dev), xpos=torch.empty(N, s.nbody, 3, device=dev),
                       xmat=torch.empty(N, s.nbody, 9, device=dev))
        if self._contact_outputs:
            out.update(contact_dist=torch.empty(N, s.ncon, device=dev), contact_pos=torch.empty(N, s.ncon, 3, device=dev),
                       contact_frame=torch.empty(N, s.ncon, 3, 3, device=dev))
        return out

    def contact(self, pipeline_state: PipelineState) -> Contact:
        """The brax-style `Contact` of a pipeline state produced with `contact_outputs=True`."""
        if pipeline_state.contact_dist is None:
            raise ValueError("build the env with contact_outputs=True to get the contact geometry")
        m, dev, nc = self.sys.model, self.device, self.sys.ncon
        t = lambda name, w: torch.from_numpy(m.table(name).reshape(nc, w) if w > 1 else m.table(name)).to(dev)
        i32 = lambda a: torch.from_numpy(a.astype("int32")).to(dev)
        z = torch.zeros(nc, device=dev)
        return Contact(dist=pipeline_state.contact_dist, pos=pipeline_state.contact_pos, frame=pipeline_state.contact_frame,
                       includemargin=z, friction=t("con_friction", 5), solref=t("con_solref", 2), solreffriction=torch.zeros(nc, 2, device=dev),
                       solimp=t("con_solimp", 5), geom1=i32(self.sys.contact_geom1), geom2=i32(self.sys.contact_geom2),
                       link_idx=(i32(self.sys.contact_link_idx[0]), i32(self.sys.contact_link_idx[1])), elasticity=z.clone())

    def pipeline_init(self, q: torch.Tensor, qd: torch.Tensor) -> PipelineState:
        N, s, dev = self.num_envs, self.sys, self.device
        st = dict(qpos=q.to(dev, torch.float32).contiguous().clone(), qvel=qd.to(dev, torch.float32).contiguous().clone(),
                  act=torch.zeros(N, s.na, device=dev), qacc_warmstart=torch.zeros(N, s.nv, device=dev))
        out = self._alloc_outputs()
        self._batch.pipeline_init(st, out)
        return PipelineState(**st, **out)

    def pipeline_step(self, pipeline_state: PipelineState, action: torch.Tensor) -> PipelineState:
        st_in = dict(qpos=pipeline_state.qpos, qvel=pipeline_state.qvel, act=pipeline_state.act,
                     qacc_warmstart=pipeline_state.qacc_warmstart)
        st = {k: torch.empty_like(v) for k, v in st_in.items()}      # out of place: the argument stays valid
        out = self._alloc_outputs()
        self._rebalance()
        self._batch.pipeline_step_to(st_in, st, action.to(self.device, torch.float32).contiguous(), self._n_frames, out)
        return PipelineState(**st, **out)
