"""Shared by tests/test_grad_clip_cpu.py and tests/test_gpu_grad_clip.py: the float64 reference of one clipped-Adam step on flat arrays and
the per-element bound a float32 evaluation of the rule must keep to it.

The bound counts the roundings of the rule (training/optim.py), u = eps32 / 2 each, to first order, from identical float32 inputs g, m0, v0,
p0.  The scale s is a float32 quotient of two float32 numbers in the rule itself, so reference and implementation hold the same s.

    g^ = s g                                     1 rounding (none where s = 1)
    m  = b1 m0 + (1 - b1) g^                     b1 and 1 - b1 as float32 (1 each), two products, g^, the sum:
                                                 |dm| <= 3u (|b1 m0| + |(1 - b1) g^|) + u |m|  <=  4u Am,   Am = |b1 m0| + |(1 - b1) g^|
    v  = b2 v0 + (1 - b2) g^ g^                  g^ twice (2), the square, 1 - b2, its product: 5u on that term; b2, its product: 2u on the
                                                 other; the sum: 1.  All terms are >= 0:  |dv| <= 6u v
    mh = m / bc1                                 bc1 as float32, the quotient:  |dmh| <= (|dm| + 2u |m|) / bc1  <=  6u Am / bc1
    d  = sqrt(v / bc2) + eps                     bc2, the quotient: 8u on v / bc2; the root halves it and adds 1: 5u; eps as float32 and the
                                                 sum (terms >= 0): |dd| <= 6u d
    q  = lr mh / d                               lr as float32, product, quotient, d:  |dq| <= lr |dmh| / d + 9u |q|
    p  = p0 - q                                  the difference:  |dp| <= u |p| + 9u |q| + 6u lr Am / (bc1 d)

In units of eps32 = 2u:  m: 2 Am;  v: 3 v;  p: 0.5 |p| + 4.5 |q| + 3 lr Am / (bc1 d).  A fused multiply-add only removes roundings.  The
bounds assume correctly rounded float32 division and square root (hipcc's and torch's default)."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
B1, B2, EPS = 0.9, 0.999, 1e-8


def reference_step(p0, g, m0, v0, t0, lr, max_grad_norm):
    """One step of the rule in float64 on flat float32 arrays (the restatement of `optim.clipped_adam_reference` goes through that function:
    this wrapper only flattens) -> dict(p, m, v, t, norm, scale, skipped, bound_p, bound_m, bound_v), the bounds per element, absolute."""
    from rodent_amd.training import optim
    p, m, v, t, info = optim.clipped_adam_reference([p0], [g], [m0], [v0], t0, lr=lr, max_grad_norm=max_grad_norm, betas=(B1, B2), eps=EPS)
    out = dict(p=p[0], m=m[0], v=v[0], t=t, **info)
    if not info["skipped"]:
        g64, s = np.asarray(g, np.float64), info["scale"]
        gh = g64 if s == 1.0 else s * g64
        Am = np.abs(B1 * np.asarray(m0, np.float64)) + np.abs((1.0 - B1) * gh)
        bc1, bc2 = 1.0 - B1 ** t, 1.0 - B2 ** t
        d = np.sqrt(out["v"] / bc2) + EPS
        q = lr * (out["m"] / bc1) / d
        out["bound_m"] = EPS32 * 2.0 * Am
        out["bound_v"] = EPS32 * 3.0 * out["v"]
        out["bound_p"] = EPS32 * (0.5 * np.abs(out["p"]) + 4.5 * np.abs(q) + 3.0 * lr * Am / (bc1 * d))
        # what torch.nn.utils.clip_grad_norm_ adds when it clips: its scale is max / (norm + 1e-6), a relative 1e-6 / norm on g^
        delta = 1e-6 / out["norm"] if (s < 1.0 and out["norm"] > 0) else 0.0
        out["torch_extra_m"] = delta * np.abs((1.0 - B1) * gh)
        out["torch_extra_v"] = 2.0 * delta * (1.0 - B2) * gh * gh
        out["torch_extra_p"] = delta * (lr * np.abs((1.0 - B1) * gh) / (bc1 * d) + np.abs(q))
    return out


def shares(got_p, got_m, got_v, ref, extra=False):
    """Largest |got - ref| / bound over the elements, for p, m, v (0 / 0 counts as 0).  `extra`: the bound torch's clip needs."""
    out = []
    for key, got in (("p", got_p), ("m", got_m), ("v", got_v)):
        b = ref["bound_" + key] + (ref["torch_extra_" + key] if extra else 0.0)
        err = np.abs(np.asarray(got, np.float64) - ref[key])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0.0, 0.0, err / b)
        out.append(float(r.max()) if r.size else 0.0)
    return out
