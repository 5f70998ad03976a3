"""Float64 reference and elementwise bound for mi355x_sd_ancestral_update (csrc/misc.hip ancestral_kernel / ancestral_rescale_kernel):
one step of ancestral Euler sampling -- guidance combine, guidance rescale, prev = a x + b e + c z -- in one launch. A sibling of
tests/multistep_bounds.py, whose guided model output (guided(): E and its bound e_E, from tests/guidance_bounds.py) and check() it
imports: |out - ref| <= 2 u |ref| + e for an fp32 store, u = 2^-24, over EVERY element.

What the kernel computes per element, in this order (coef = (a, b, c) fp32, t = eps_text, u = eps_uncond, z = noise):
    e   = fma(gs, fl(t - u), u)                        (no eps_text: e = u, exactly)
    E   = fl(e * k)                                    guidance_rescale > 0 only; k of guidance_bounds (per sample, same tree sums)
    s   = fl(fl(a x) + fl(b E))
    out = fl(s + fl(c z))                              c == 0: out = s and z is NOT read
(which products fuse into the sums is the compiler's choice: a fused product drops one rounding, the bound covers both).

The bound (1.01 absorbs second-order products of u terms, as in guidance_bounds). x and z are read, E is computed (e_E):
  * the computed E enters through b: |b| e_E.
  * roundings per term, each at that term's magnitude. c != 0: a x passes its product, the first sum and the last sum (3), b E the
    same three, c z its product and the last sum (2):
        e_out = |b| e_E + 1.01 u (3 (|a x| + |b| (|E| + e_E)) + 2 |c z|)
    c == 0: there is no last sum, a x and b E pass two roundings each and z does not appear:
        e_out = |b| e_E + 1.01 u * 2 (|a x| + |b| (|E| + e_E))
    The reference at c == 0 does not read z either: a kernel that forms 0 * z over a NaN plane leaves the bound (inf), one that rounds z
    to 8 mantissa bits before use leaves it by |c z| 2^-9 against 2 u |c z| (tests/test_ancestral_bounds.py injects both).

accumulated() carries the bound through a loop against the generic loop (scheduler.step) run in float64 on the model outputs and the
noise planes the fused loop saw. With (a, b, c) the float64 coefficients, x32 the fp32 table entries, x_i the fused loop's latents, ref
the kernel's float64 value at the fused inputs:
    E_x' = |a| E_x + |a32 - a| |x_i| + |b32 - b| |E| + |c32 - c| |z| + (2 u |ref| + e_out)
E_0 = u |x_0| if the start was scaled by init_noise_sigma != 1 (one fp32 product).
"""
import torch

from paddlemix_amd.schedulers import EulerAncestralDiscreteScheduler
from tests.guidance_bounds import RESIDENT
from tests.multistep_bounds import guided
from tests.rowmap_bounds import U32, check
from tests.step_pieces import base_inputs

SCHED = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def schedule_rows(steps=20, **kw):
    """(a, b, c) of every step of a schedule, as Python floats"""
    sch = EulerAncestralDiscreteScheduler(**dict(SCHED, **kw))
    sch.set_timesteps(steps)
    return [sch.ancestral_coefficients(t) for t in sch.timesteps]


ROWS_V, ROWS_EPS = schedule_rows(prediction_type="v_prediction"), schedule_rows()
ROW = {"mid": ROWS_V[10], "eps": ROWS_EPS[10], "last": ROWS_V[-1]}   # a != 1, b, c != 0; a == 1; c == 0
POINTERS = ("x", "eu", "et", "z", "out")
CASES = {   # name: batch, per_sample and what differs from gs = 7.5, gr = 0, row "mid", CFG, random inputs, aligned pointers
    "b2 n512 vectors": dict(batch=2, n=512),
    "b2 n512 epsilon row": dict(batch=2, n=512, row="eps"),
    "b2 n512 no eps_text": dict(batch=2, n=512, cfg=False),
    "b1 n252 below one block": dict(batch=1, n=4 * 9 * 7),
    "b1 n251 vectors + tail": dict(batch=1, n=251),
    "b1 n251 no eps_text": dict(batch=1, n=251, cfg=False),
    "b1 n1": dict(batch=1, n=1),
    **{f"b2 n512 {p} offset one element": dict(batch=2, n=512, misalign=p) for p in POINTERS},
    "b2 n512 out=x": dict(batch=2, n=512, alias=True),
    "b2 n512 c0 NaN noise": dict(batch=2, n=512, row="last", nan_noise=True),
    "b1 n251 c0 NaN noise": dict(batch=1, n=251, row="last", nan_noise=True),
    "b2 n512 c0 null noise": dict(batch=2, n=512, row="last", nan_noise=True, null_noise=True),
    "b2 n1024 rescale": dict(batch=2, n=1024, gr=0.7),
    "b1 n2 smallest rescale": dict(batch=1, n=2, gr=0.7),
    "b3 n1023 odd rescale": dict(batch=3, n=1023, gr=0.7),
    "b2 n1024 rescale offset 64": dict(batch=2, n=1024, gr=0.7, kind="offset"),
    "b2 n1024 rescale out=x": dict(batch=2, n=1024, gr=0.7, alias=True),
    "b2 n1024 rescale c0 NaN noise": dict(batch=2, n=1024, gr=0.7, row="last", nan_noise=True),
    "b2 n1024 rescale c0 null noise": dict(batch=2, n=1024, gr=0.7, row="last", nan_noise=True, null_noise=True),
    "b2 n32768 rescale resident": dict(batch=2, n=RESIDENT, gr=0.7),
    "b2 n32772 rescale loop form": dict(batch=2, n=RESIDENT + 4, gr=0.7),
    "b2 n32772 rescale loop form c0 NaN noise": dict(batch=2, n=RESIDENT + 4, gr=0.7, row="last", nan_noise=True),
}


def inputs(name):
    """dict(x, eu, et (None: no guidance), z, coef, gs, gr) of a case: CPU fp32 [batch, n], seeded by the name"""
    s = CASES[name]
    g, shape, x, eu, et = base_inputs(name, s)
    z = torch.randn(shape, generator=g)
    if s.get("nan_noise"):
        z = torch.full(shape, float("nan"))
    return dict(x=x, eu=eu, et=et, z=z, coef=torch.tensor(ROW[s.get("row", "mid")], dtype=torch.float32),
                gs=s.get("gs", 7.5), gr=s.get("gr", 0.0))


def ancestral_update(x, eu, et, z, coef, gs, gr, depth=None):
    """x, eu, et (or None), z fp32 [batch, n]; coef fp32 (a, b, c); gs, gr as the C ABI passes them ->
    dict(out, e_out, E, cz) float64 [batch, n]"""
    a, b, c = coef.double().tolist()
    E, e_E = guided(eu, et, gs, gr, depth)
    ax = a * x.double()
    out = ax + b * E
    det = ax.abs() + abs(b) * (E.abs() + e_E)
    cz = torch.zeros_like(out)
    if c != 0.0:
        cz = c * z.double()
        out = out + cz
        e_out = abs(b) * e_E + 1.01 * U32 * (3 * det + 2 * cz.abs())
    else:
        e_out = abs(b) * e_E + 1.01 * U32 * 2 * det
    return dict(out=out, e_out=e_out, E=E, cz=cz)


def ratio(v, out):
    """worst |out - ref| / bound of a case's inputs (inputs()) over every element"""
    r = ancestral_update(v["x"], v["eu"], v["et"], v["z"], v["coef"], v["gs"], v["gr"])
    return check(out.reshape(v["x"].shape), r["out"], r["e_out"])


def accumulated(xs, zs, outs, coef64, gs, gr, cfg=True, sigma0=1.0):
    """The bound on |fused latents - float64 generic latents| after every step of a loop whose model outputs and noise were replayed.
    xs[i]: the fused loop's fp32 latents [B, ...] before step i; zs[i]: the fp32 noise plane of step i; outs[i]: its fp32 model output
    ([2 B, ...] = [uncond, text] with cfg); coef64: (a, b, c) per step as Python floats -> list of float64 bounds shaped like the latents"""
    E_x = (U32 * xs[0].double().abs() if sigma0 != 1.0 else torch.zeros_like(xs[0], dtype=torch.float64)).flatten(1)
    res = []
    for x, z, o, c64 in zip(xs, zs, outs, coef64):
        Bn = x.shape[0]
        c32 = torch.tensor(c64, dtype=torch.float32)
        xf, zf = x.flatten(1), z.flatten(1)
        r = ancestral_update(xf, o[:Bn].flatten(1), o[Bn:].flatten(1) if cfg else None, zf, c32, gs, gr if cfg else 0.0)
        da, db, dc = (abs(p - q) for p, q in zip(c32.double().tolist(), c64))
        E_x = abs(c64[0]) * E_x + da * xf.double().abs() + db * r["E"].abs() + (dc * zf.double().abs() if c64[2] != 0.0 else 0.0) \
            + 2 * U32 * r["out"].abs() + r["e_out"]
        res.append(E_x.reshape(x.shape))
    return res
