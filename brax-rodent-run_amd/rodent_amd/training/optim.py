"""Adam behind a global-norm clip, with non-finite updates skipped: `optax.chain(optax.clip_by_global_norm(max_grad_norm), optax.adam(lr))`
[UP brax.training.agents.ppo.train, `max_grad_norm`] on the flat gradient buffer of `distributed.FlatGrads`.

The rule of one step (`clipped_adam_reference` restates it in numpy float64):

    norm = float32(sqrt(sum_i g_i^2))         squares summed in float64 over ALL parameters, rounded to float32 once
    norm not finite:  the step is SKIPPED     parameters, both moments and t keep their bits, `skipped` goes up
    s  = 1 if norm <= max_grad_norm else max_grad_norm / norm
    g^ = g where s = 1 (unscaled, not multiplied by a computed 1), else s * g          one float32 multiply
    t += 1;  m = b1 m + (1 - b1) g^;  v = b2 v + (1 - b2) g^2
    p -= lr * (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)                           eps outside the root (optax)

The skip is an EXTENSION over optax, which would carry a NaN gradient into the moments and from there into every parameter for the rest
of the run; it is the learner's counterpart of the env's `bad_state_max`.  The sum is taken in float64, so a non-finite norm means that
some gradient element is NaN or +-inf (or that the norm itself is beyond float32's range).

On a GPU the step is three launches of csrc/rr_ppo.h (`hip.clipped_adam_step`) which read t, the hyper-parameters and the statistics from
device memory, so a captured HIP graph replays them; on the CPU the same rule in plain torch (the gloo data-parallel path, the CPU tests).
The parameters stay where they are: the kernels reach them through a table of (pointer, offset in the flat gradient, numel).

Two controls driven by the minibatch's approx_kl sit in front of that step when asked for (`kl_control_rule` is the rule; the finalisation
kernel of `rr_clipped_adam_step_kl`, the CPU step and the tests restate it): the `target_kl` stop of Spinning Up / Stable-Baselines3 and the
KL-adaptive learning rate of rsl_rl.  The KL is the first element behind the parameters in the flat gradient buffer
(`FlatGrads(params, extra=4)`), so the ranks' all-reduce averages it with the gradients and every rank decides from identical bits."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

MAX_TENSORS = 64
# the device state block (doubles; include/rodent_rr.h, rr_clipped_adam_step)
ST_T, ST_NORM, ST_SCALE, ST_SKIP, ST_BC1, ST_BC2, ST_NORM_SUM, ST_NORM_MAX, ST_APPLIED, ST_CLIPPED, ST_SKIPPED = 0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12
ST_STOP, ST_KL, ST_STOPPED = 6, 7, 13     # rr_clipped_adam_step_kl: sticky stop flag, the last KL, stopped updates since the last clear
STATE_DOUBLES = 16
CFG_DOUBLES = 8                       # lr, b1, b2, eps, max_grad_norm


def check_max_grad_norm(max_grad_norm) -> float:
    """A float > 0 (`inf` allowed); anything else raises ValueError."""
    if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float, np.integer, np.floating)):
        raise ValueError(f"max_grad_norm must be None or a number > 0 (inf allowed), got {max_grad_norm!r}")
    x = float(max_grad_norm)
    if not x > 0.0:                   # also NaN
        raise ValueError(f"max_grad_norm must be None or a number > 0 (inf allowed), got {max_grad_norm!r}")
    return x


# target_kl stops at 1.5 x the target: the convention of Spinning Up's PPO and of Stable-Baselines3, taken over as it is
KL_STOP_FACTOR = 1.5
# rsl_rl's adaptive schedule: lr / 1.5 above 2 x desired_kl, lr * 1.5 below desired_kl / 2.  Its defaults, untuned for this project
KL_LR_FACTOR = 1.5
DESIRED_KL_DEFAULT = 0.01
LR_BOUNDS_DEFAULT = (1e-5, 1e-2)


def check_target_kl(target_kl) -> float:
    """A finite float > 0; anything else raises ValueError."""
    if isinstance(target_kl, bool) or not isinstance(target_kl, (int, float, np.integer, np.floating)) or not (0.0 < float(target_kl) < math.inf):
        raise ValueError(f"target_kl must be None or a finite number > 0, got {target_kl!r}")
    return float(target_kl)


def check_adaptive_kl(learning_rate, desired_kl, learning_rate_bounds):
    """(desired_kl, lo, hi) as floats: desired_kl finite > 0, 0 < lo <= learning_rate <= hi finite; anything else raises ValueError."""
    num = lambda x: not isinstance(x, bool) and isinstance(x, (int, float, np.integer, np.floating))
    if not num(desired_kl) or not (0.0 < float(desired_kl) < math.inf):
        raise ValueError(f"desired_kl must be a finite number > 0, got {desired_kl!r}")
    try:
        lo, hi = learning_rate_bounds
    except (TypeError, ValueError):
        raise ValueError(f"learning_rate_bounds must be a pair (lo, hi), got {learning_rate_bounds!r}") from None
    if not num(lo) or not num(hi) or not (0.0 < float(lo) <= float(hi) < math.inf):
        raise ValueError(f"learning_rate_bounds must be 0 < lo <= hi < inf, got {learning_rate_bounds!r}")
    if not float(lo) <= float(learning_rate) <= float(hi):
        raise ValueError(f"learning_rate {learning_rate!r} lies outside learning_rate_bounds {learning_rate_bounds!r}")
    return float(desired_kl), float(lo), float(hi)


def kl_control_rule(kl: float, lr: float, stopped: bool, *, stop_threshold: float = 0.0, desired_kl: float = 0.0, lr_lo: float = 0.0,
                    lr_hi: float = 0.0, norm_finite: bool = True):
    """What one update does with the minibatch's approx_kl, measured before the update: (lr, stopped, applied), in float64.

    stopped already (sticky until `ClippedAdam.begin_training_step`): not applied, nothing moves.  stop_threshold > 0 (= 1.5 x target_kl)
    and not kl <= stop_threshold -- a NaN KL included: stop; this update and every later one of the training step is not applied.  A
    gradient norm that is not finite: skipped, the learning rate is left alone.  Otherwise, with desired_kl > 0, rsl_rl's schedule acts
    on the learning rate BEFORE the update: kl > 2 desired_kl: lr = max(lr_lo, lr / 1.5); 0 < kl < desired_kl / 2: lr = min(lr_hi, lr * 1.5);
    and the update is applied at that lr.  `kl` is the float32-rounded KL as a float64 number; 0 switches a control off."""
    kl, lr = float(kl), float(lr)
    if stopped:
        return lr, True, False
    if stop_threshold > 0.0 and not kl <= stop_threshold:
        return lr, True, False
    if not norm_finite:
        return lr, False, False
    if desired_kl > 0.0:
        if kl > 2.0 * desired_kl:
            lr = max(float(lr_lo), lr / KL_LR_FACTOR)
        elif 0.0 < kl < 0.5 * desired_kl:
            lr = min(float(lr_hi), lr * KL_LR_FACTOR)
    return lr, False, True


def clipped_adam_reference(params: Sequence[np.ndarray], grads: Sequence[np.ndarray], m: Sequence[np.ndarray], v: Sequence[np.ndarray], t: int, *,
                           lr: float, max_grad_norm: float, betas=(0.9, 0.999), eps: float = 1e-8):
    """The rule in numpy float64 on lists of arrays.  Returns (params, m, v, t, info) with info = dict(norm, scale, skipped); the inputs
    are not modified.  `norm` is the float32-rounded norm the rule compares with `max_grad_norm` (as a float64 number)."""
    b1, b2 = float(betas[0]), float(betas[1])
    g = [np.asarray(x, dtype=np.float64) for x in grads]
    p = [np.array(x, dtype=np.float64) for x in params]
    m = [np.array(x, dtype=np.float64) for x in m]
    v = [np.array(x, dtype=np.float64) for x in v]
    with np.errstate(all="ignore"):
        norm = float(np.float32(np.sqrt(sum(float(np.sum(x * x)) for x in g))))
    if not math.isfinite(norm):
        return p, m, v, int(t), dict(norm=norm, scale=1.0, skipped=True)
    mx = float(np.float32(max_grad_norm))
    s = 1.0 if norm <= mx else float(np.float32(mx) / np.float32(norm))
    t = int(t) + 1
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    for k in range(len(p)):
        gh = g[k] if s == 1.0 else s * g[k]
        m[k] = b1 * m[k] + (1.0 - b1) * gh
        v[k] = b2 * v[k] + (1.0 - b2) * gh * gh
        p[k] = p[k] - lr * (m[k] / bc1) / (np.sqrt(v[k] / bc2) + eps)
    return p, m, v, t, dict(norm=norm, scale=s, skipped=False)


class ClippedAdam:
    """`ClippedAdam(params, flat, lr, max_grad_norm)`: `params` the parameter tensors in `FlatGrads` order, `flat` the `FlatGrads` (or its flat
    float32 gradient tensor) their gradients live in.  `step()` applies one update from the gradient as it stands in `flat` -- after the ranks'
    all-reduce, so every rank computes the same values.  `stats(clear=)` reads the counters of the steps since the last clear (one small
    device-to-host copy: call it after a synchronise, not inside the update loop).

    `target_kl` and / or `desired_kl` with `learning_rate_bounds` switch the KL controls on (`kl_control_rule`).  The step then reads the
    minibatch's approx_kl from the first extra slot of `flat`, a `FlatGrads(params, extra=...)`; the norm is taken over the parameters'
    elements alone.  `begin_training_step()` clears the sticky stop
    flag, `stopped` reads it (one 8-byte copy), `learning_rate` reads the current rate."""

    def __init__(self, params, flat, lr: float, max_grad_norm: float, betas=(0.9, 0.999), eps: float = 1e-8, *, target_kl=None, desired_kl=None,
                 learning_rate_bounds=None):
        self.params = [p for p in params]
        self.flat = flat.flat if hasattr(flat, "flat") else flat
        n_params = sum(p.numel() for p in self.params)
        kl = None
        if getattr(flat, "extra", 0):                        # the tail behind the parameters is not part of the gradient
            kl = self.flat[n_params:n_params + 1]
            self.flat = self.flat[:n_params]
        self.kl_cfg = None
        if target_kl is not None or desired_kl is not None:
            thr = KL_STOP_FACTOR * check_target_kl(target_kl) if target_kl is not None else 0.0
            des, lo, hi = check_adaptive_kl(lr, desired_kl, learning_rate_bounds) if desired_kl is not None else (0.0, 0.0, 0.0)
            if kl is None:
                raise ValueError("ClippedAdam: the KL controls read the KL from the slot behind the gradients: pass a FlatGrads(params, extra=4)")
            self.kl_cfg = (thr, des, lo, hi)
        self.kl = kl if self.kl_cfg is not None else None
        self.target_kl, self.desired_kl, self.learning_rate_bounds = target_kl, desired_kl, learning_rate_bounds
        self.max_grad_norm = check_max_grad_norm(max_grad_norm)
        if not (lr >= 0.0 and math.isfinite(lr)) or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or not eps >= 0.0:
            raise ValueError(f"ClippedAdam: bad hyper-parameters lr={lr!r} betas={betas!r} eps={eps!r}")
        if not self.params or len(self.params) > MAX_TENSORS:
            raise ValueError(f"ClippedAdam: 1 .. {MAX_TENSORS} parameter tensors, got {len(self.params)}")
        n = sum(p.numel() for p in self.params)
        dev = self.flat.device
        if self.flat.dtype != torch.float32 or self.flat.dim() != 1 or self.flat.numel() != n or not self.flat.is_contiguous():
            raise ValueError(f"ClippedAdam: the flat gradient must be a contiguous float32 vector of {n} elements (the parameters' total)")
        for p in self.params:
            if p.dtype != torch.float32 or p.device != dev or not p.is_contiguous():
                raise ValueError("ClippedAdam: parameters must be contiguous float32 tensors on the flat gradient's device")
        self.lr, self.betas, self.eps, self.n = float(lr), (float(betas[0]), float(betas[1])), float(eps), n
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self.offsets = np.concatenate([[0], np.cumsum([p.numel() for p in self.params])]).astype(np.int64)
        self.state = {}                       # filled by the first step, like torch.optim.Optimizer.state
        self._warned = False
        self._dev = None
        if dev.type == "cuda":
            from .. import hip
            self._dev = hip.ClippedAdamBuffers(self.params, self.flat, self.exp_avg, self.exp_avg_sq,
                                               lr=self.lr, b1=self.betas[0], b2=self.betas[1], eps=self.eps, max_grad_norm=self.max_grad_norm,
                                               kl=self.kl, kl_cfg=self.kl_cfg)
        else:
            self._st = np.zeros(STATE_DOUBLES, dtype=np.float64)
            self._lr = self.lr                # the current rate (the adaptive schedule moves it; `self.lr` stays the constructor's)

    # ------------------------------------------------------------------ the step
    def step(self):
        if self._dev is not None:
            self._dev.step()
        else:
            self._cpu_step()
        if not self.state:
            self.state = {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "device_state": self._dev.state if self._dev is not None else self._st}

    @torch.no_grad()
    def _cpu_step(self):
        st, g = self._st, self.flat
        kl = None
        if self.kl_cfg is not None:                                   # the stop first: while the flag is set nothing but its counter moves
            thr, des, lo, hi = self.kl_cfg
            kl = float(self.kl)
            _, stop, _ = kl_control_rule(kl, self._lr, st[ST_STOP] != 0.0, stop_threshold=thr)
            if stop:
                if st[ST_STOP] == 0.0:
                    st[ST_KL] = kl
                st[ST_STOP] = st[ST_SKIP] = 1.0
                st[ST_STOPPED] += 1.0
                return
            st[ST_KL] = kl
        norm = g.double().square().sum().sqrt().float()              # float64 sum, rounded to float32 once
        st[ST_NORM] = float(norm)
        if kl is not None:
            self._lr, _, _ = kl_control_rule(kl, self._lr, False, stop_threshold=thr, desired_kl=des, lr_lo=lo, lr_hi=hi,
                                             norm_finite=bool(torch.isfinite(norm)))
        if not bool(torch.isfinite(norm)):
            st[ST_SKIP] = 1.0
            st[ST_SKIPPED] += 1.0
            return
        mx = torch.tensor(self.max_grad_norm, dtype=torch.float32)
        clipped = bool(norm > mx)
        s = mx / norm if clipped else torch.ones((), dtype=torch.float32)
        clipped = clipped and bool(s < 1.0)
        gh = g * s if clipped else g                                  # below or at the threshold: the gradient itself
        t = int(st[ST_T]) + 1
        b1, b2 = self.betas
        bc1, bc2 = np.float32(1.0 - b1 ** t), np.float32(1.0 - b2 ** t)
        self.exp_avg.mul_(b1).add_(gh, alpha=1.0 - b1)
        self.exp_avg_sq.mul_(b2).addcmul_(gh, gh, value=1.0 - b2)
        upd = (self.exp_avg / float(bc1)) / ((self.exp_avg_sq / float(bc2)).sqrt_() + self.eps)
        for k, p in enumerate(self.params):
            p.data.add_(upd[self.offsets[k]:self.offsets[k + 1]].view_as(p), alpha=-self._lr)
        st[ST_T], st[ST_SCALE], st[ST_SKIP], st[ST_BC1], st[ST_BC2] = t, float(s), 0.0, float(bc1), float(bc2)
        st[ST_NORM_SUM] += float(norm)
        st[ST_NORM_MAX] = max(st[ST_NORM_MAX], float(norm))
        st[ST_APPLIED] += 1.0
        st[ST_CLIPPED] += 1.0 if clipped else 0.0

    # ------------------------------------------------------------------ state
    def _state_host(self) -> np.ndarray:
        return self._dev.state.cpu().numpy() if self._dev is not None else self._st

    @property
    def t(self) -> int:
        """Applied updates so far (Adam's step count; a skipped update does not count).  Reads the device."""
        return int(self._state_host()[ST_T])

    def begin_training_step(self):
        """Clear the sticky stop flag of `target_kl`: the start of a training step's learner phase."""
        if self._dev is not None:
            self._dev.state[ST_STOP].zero_()
        else:
            self._st[ST_STOP] = 0.0

    @property
    def stopped(self) -> bool:
        """The stop flag of `target_kl`.  On a GPU one 8-byte device-to-host copy (it waits for the stream): once per pass, not per update."""
        return bool(self._dev.state[ST_STOP].item() != 0.0) if self._dev is not None else bool(self._st[ST_STOP] != 0.0)

    @property
    def learning_rate(self) -> float:
        """The rate the next update uses (the adaptive schedule moves it).  Reads the device."""
        return float(self._dev.cfg[0].item()) if self._dev is not None else float(self._lr)

    def stats(self, clear: bool = True) -> dict:
        """Counters since the last clear: grad_norm (mean pre-clip norm over the applied updates), grad_norm_max (over the applied updates),
        grad_clip_share (applied updates with s < 1), skipped_updates, applied_updates; with the KL controls also stopped_updates (not
        applied because of `target_kl`), last_kl (the KL the last deciding update saw) and learning_rate.  `clear` zeroes the counters'
        slots 8 .. 13 of the state block, the stopped-updates slot included whether or not a KL control is on."""
        st = self._state_host()
        applied, skipped = int(st[ST_APPLIED]), int(st[ST_SKIPPED])
        out = {"grad_norm": float(st[ST_NORM_SUM]) / applied if applied else 0.0, "grad_norm_max": float(st[ST_NORM_MAX]),
               "grad_clip_share": float(st[ST_CLIPPED]) / applied if applied else 0.0, "skipped_updates": skipped, "applied_updates": applied}
        if self.kl_cfg is not None:
            out.update(stopped_updates=int(st[ST_STOPPED]), last_kl=float(st[ST_KL]), learning_rate=self.learning_rate)
        if clear:
            if self._dev is not None:
                self._dev.state[ST_NORM_SUM:ST_STOPPED + 1].zero_()
            else:
                st[ST_NORM_SUM:ST_STOPPED + 1] = 0.0
        return out

    def state_dict(self) -> dict:
        """`lr` (the current rate), `kl_stop` and `stopped` are always present, also for an optimiser built without a KL control (the
        constructor's rate, False, 0); on a GPU `lr` is one more small device read."""
        st = self._state_host()
        return {"t": int(st[ST_T]), "exp_avg": self.exp_avg.detach().clone(), "exp_avg_sq": self.exp_avg_sq.detach().clone(),
                "stats": [float(x) for x in st[ST_NORM_SUM:ST_SKIPPED + 1]],
                "lr": self.learning_rate, "kl_stop": bool(st[ST_STOP] != 0.0), "stopped": float(st[ST_STOPPED]),
                "hyper": {"lr": self.lr, "betas": self.betas, "eps": self.eps, "max_grad_norm": self.max_grad_norm}}

    def load_state_dict(self, sd: dict):
        """Moments, t, the counters and -- where the dict has them -- the current learning rate and the stop flag; the other
        hyper-parameters stay the constructor's (the dict carries them for the record)."""
        if sd["exp_avg"].numel() != self.n or sd["exp_avg_sq"].numel() != self.n:
            raise ValueError(f"ClippedAdam.load_state_dict: moments of {sd['exp_avg'].numel()} elements, expected {self.n}")
        self.exp_avg.copy_(sd["exp_avg"].reshape(-1))
        self.exp_avg_sq.copy_(sd["exp_avg_sq"].reshape(-1))
        new = np.zeros(STATE_DOUBLES, dtype=np.float64)
        new[ST_T] = int(sd["t"])
        new[ST_NORM_SUM:ST_SKIPPED + 1] = sd.get("stats", [0.0] * 5)
        new[ST_STOP] = new[ST_SKIP] = 1.0 if sd.get("kl_stop", False) else 0.0
        new[ST_STOPPED] = sd.get("stopped", 0.0)
        lr = float(sd.get("lr", self.lr))
        if self._dev is not None:
            self._dev.state.copy_(torch.from_numpy(new))
            self._dev.cfg[0] = lr
        else:
            self._st[:] = new
            self._lr = lr
        if not self.state and int(sd["t"]):
            self.state = {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "device_state": self._dev.state if self._dev is not None else self._st}
