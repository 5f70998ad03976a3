"""Float64 reference and elementwise bound for mi355x_sd_dpm2_update (csrc/step_tail.hip MidpointStep): one model evaluation of a
two-stage midpoint step (DPM2, DPM2 a) -- guidance combine, guidance rescale, the derivative, the update, the noise term and the parked
sample -- in one launch. A sibling of tests/heun_bounds.py and tests/ancestral_bounds.py: the guided model output (guided(): E and its
bound e_E) comes from tests/multistep_bounds.py, check() and U32 from tests/rowmap_bounds.py: |out - ref| <= 2 u |ref| + e for an fp32
store, u = 2^-24, over EVERY element of out; the parked sample S is a copy and must be exact.

What the kernel computes per element, in this order (coef = (p, q, h, c, second) fp32, S the parked sample, z the noise):
    E   = the guided (and rescaled) model output                    e_E of multistep_bounds.guided
    d   = fl(fl(p x) + fl(q E))                                     p == 0: d = fl(q E), x does not enter
    second == 0:  out = fl(x + fl(h d))      S <- x (bit copy)      S and z are NOT read
    second != 0:  s   = fl(S + fl(h d))      S is NOT written
                  out = fl(s + fl(c z))      c == 0: out = s and z is NOT read
(which products fuse into the sums is the compiler's choice: a fused product drops one rounding, the bound covers both).

The bound (1.01 absorbs second-order products of u terms, as in guidance_bounds). x, S and z are read, E is computed (e_E):
  * d, as in heun_bounds: the computed E enters through q. p != 0: p x and q E pass their product and the sum (2 roundings each);
    p == 0: q E passes its product alone (1):
        e_d = |q| e_E + 1.01 u r_d (|p x| + |q| (|E| + e_E)),  r_d = 2 (p != 0) or 1 (p == 0).
  * stage 1, and stage 2 at c == 0, with B the base (x or S): B passes the sum (1), h d its product and the sum (2):
        e_out = |h| e_d + 1.01 u (|B| + 2 |h| (|d| + e_d)).     In stage 1 S must equal x bit for bit (its bound is 0).
  * stage 2 at c != 0: there is a second sum. S passes both sums (2), h d its product and both sums (3), c z its product and the last
    sum (2):
        e_out = |h| e_d + 1.01 u (2 |S| + 3 |h| (|d| + e_d) + 2 |c z|).
    The reference of a row reads only what that row may read: a stage 1 that forms a term over a NaN S, any row that forms 0 * z over a
    NaN plane, or a stage 2 at p == 0 that forms 0 * x over a NaN x leaves the bound (inf); a stage 2 that starts from x instead of S
    is off by |x - S|; a z rounded to 8 mantissa bits before use by |c z| 2^-9 against 2 u |c z| (tests/test_dpm2_bounds.py injects
    them).

accumulated() carries the bound through a loop against the generic loop (scheduler.step) run in float64 on the model outputs and the
noise planes the fused loop saw. Two errors travel: E_x of the latents and E_S of the parked sample. With (p, q, h, c) the float64
coefficients, x32 the fp32 table entries, x_i / S_i the fused loop's buffers, ref the kernel's float64 value at the fused inputs:
    dd   = |p| E_x + |p32 - p| |x_i| + |q32 - q| |E|                                      (ref d against the generic derivative)
    stage 1:  E_x' = E_x + |h| dd + |h32 - h| |d| + (2 u |ref| + e_out),   E_S' = E_x
    stage 2:  E_x' = E_S + |h| dd + |h32 - h| |d| + |c32 - c| |z| + (2 u |ref| + e_out)
E_0 = u |x_0| if the start was scaled by init_noise_sigma != 1 (one fp32 product). The float64 roundings of the generic loop's own
formulas (x0, (x - x0) / sigma, the sums) are 2^-29 of these and are not counted, as in the sibling modules.
"""
import torch

from paddlemix_amd.schedulers import KDPM2AncestralDiscreteScheduler, KDPM2DiscreteScheduler
from tests.guidance_bounds import RESIDENT
from tests.multistep_bounds import guided
from tests.rowmap_bounds import U32, check
from tests.step_pieces import base_inputs, counting

SCHED = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
CLASSES = {"dpm2": KDPM2DiscreteScheduler, "dpm2a": KDPM2AncestralDiscreteScheduler}


def scheduler(which, widen=False, **kw):
    """a counted scheduler of CLASSES[which] on the SD betas; widen: see tests/step_pieces.py counting (the ancestral class's
    float64 generic loop is handed its generator's float32 draws)"""
    return counting(CLASSES[which](**dict(SCHED, **kw)), widen and which == "dpm2a")


def schedule_rows(which, steps=20, **kw):
    """(p, q, h, c, second) of every model evaluation of a schedule (2 * steps - 1 rows), as Python floats"""
    sch = CLASSES[which](**dict(SCHED, **kw))
    sch.set_timesteps(steps)
    with sch.coefficient_walk():
        return [sch.dpm2_coefficients(t) for t in sch.timesteps]


ROWS_V, ROWS_EPS = schedule_rows("dpm2a", prediction_type="v_prediction"), schedule_rows("dpm2a")
ROWS_V0, ROWS_EPS0 = schedule_rows("dpm2", prediction_type="v_prediction"), schedule_rows("dpm2")
ROW = {"v1": ROWS_V[10], "v2": ROWS_V[11], "eps1": ROWS_EPS[10], "eps2": ROWS_EPS[11], "last": ROWS_V[-1],   # DPM2 a: c != 0 in stage 2
       "v2c0": ROWS_V0[11], "eps2c0": ROWS_EPS0[11]}                                                          # DPM2: c == 0
POINTERS = ("x", "eu", "et", "z", "S", "out")
_BOTH = (("stage 1", "v1"), ("stage 2", "v2"))
CASES = {   # name: batch, per_sample and what differs from gs = 7.5, gr = 0, CFG, random inputs and state, aligned pointers
    **{f"b2 n512 vectors {s}": dict(batch=2, n=512, row=r) for s, r in _BOTH},
    **{f"b1 n251 vectors + tail {s}": dict(batch=1, n=251, row=r) for s, r in _BOTH},
    **{f"b1 n252 below one block {s}": dict(batch=1, n=252, row=r) for s, r in _BOTH},
    **{f"b1 n1 {s}": dict(batch=1, n=1, row=r) for s, r in _BOTH},
    "b2 n512 epsilon row stage 1": dict(batch=2, n=512, row="eps1"),
    "b2 n512 epsilon row stage 2": dict(batch=2, n=512, row="eps2"),
    "b1 n251 epsilon row stage 2": dict(batch=1, n=251, row="eps2"),
    "b2 n512 last row": dict(batch=2, n=512, row="last"),
    "b2 n512 stage 2 c0": dict(batch=2, n=512, row="v2c0"),
    **{f"b2 n512 no eps_text {s}": dict(batch=2, n=512, row=r, cfg=False) for s, r in _BOTH},
    "b1 n251 no eps_text stage 1": dict(batch=1, n=251, row="v1", cfg=False),
    **{f"b2 n512 {p} offset one element {s}": dict(batch=2, n=512, row=r, misalign=p) for p in POINTERS for s, r in _BOTH},
    **{f"b2 n512 out=x {s}": dict(batch=2, n=512, row=r, alias=True) for s, r in _BOTH},
    "b2 n512 stage 1 NaN S and noise": dict(batch=2, n=512, row="v1", nan=("S", "z")),
    "b1 n251 stage 1 NaN S and noise": dict(batch=1, n=251, row="eps1", nan=("S", "z")),
    "b2 n512 stage 2 c0 NaN noise": dict(batch=2, n=512, row="v2c0", nan=("z",)),
    "b1 n251 stage 2 c0 NaN noise": dict(batch=1, n=251, row="eps2c0", nan=("z",)),
    "b2 n512 stage 2 c0 null noise": dict(batch=2, n=512, row="v2c0", nan=("z",), null_noise=True),
    "b2 n512 stage 1 null noise": dict(batch=2, n=512, row="v1", nan=("S", "z"), null_noise=True),
    "b2 n512 stage 2 p0 NaN x": dict(batch=2, n=512, row="eps2", nan=("x",)),
    "b1 n251 stage 2 p0 NaN x": dict(batch=1, n=251, row="eps2c0", nan=("x",)),
    **{f"b2 n1024 rescale {s}": dict(batch=2, n=1024, gr=0.7, row=r) for s, r in _BOTH},
    **{f"b1 n2 smallest rescale {s}": dict(batch=1, n=2, gr=0.7, row=r) for s, r in _BOTH},
    **{f"b3 n1023 odd rescale {s}": dict(batch=3, n=1023, gr=0.7, row=r) for s, r in _BOTH},
    **{f"b2 n1024 rescale offset 64 {s}": dict(batch=2, n=1024, gr=0.7, row=r, kind="offset") for s, r in _BOTH},
    "b2 n1024 rescale out=x stage 1": dict(batch=2, n=1024, gr=0.7, row="v1", alias=True),
    "b2 n1024 rescale epsilon row stage 2": dict(batch=2, n=1024, gr=0.7, row="eps2"),
    "b2 n1024 rescale stage 1 NaN S and noise": dict(batch=2, n=1024, gr=0.7, row="v1", nan=("S", "z")),
    "b2 n1024 rescale stage 2 c0 NaN noise": dict(batch=2, n=1024, gr=0.7, row="v2c0", nan=("z",)),
    "b2 n1024 rescale stage 2 c0 null noise": dict(batch=2, n=1024, gr=0.7, row="v2c0", nan=("z",), null_noise=True),
    "b2 n1024 rescale stage 2 p0 NaN x": dict(batch=2, n=1024, gr=0.7, row="eps2", nan=("x",)),
    **{f"b2 n32768 rescale resident {s}": dict(batch=2, n=RESIDENT, gr=0.7, row=r) for s, r in _BOTH},
    **{f"b2 n32772 rescale loop form {s}": dict(batch=2, n=RESIDENT + 4, gr=0.7, row=r) for s, r in _BOTH},
    "b2 n32772 rescale loop form stage 1 NaN S and noise": dict(batch=2, n=RESIDENT + 4, gr=0.7, row="v1", nan=("S", "z")),
}


def inputs(name):
    """dict(x, eu, et (None: no guidance), z, S, coef, gs, gr) of a case: CPU fp32 [batch, n], seeded by the name"""
    s = CASES[name]
    g, shape, x, eu, et = base_inputs(name, s)
    v = dict(x=x, S=3.0 * torch.randn(shape, generator=g), z=torch.randn(shape, generator=g))   # S is NOT near x: a stage 2 from x shows
    for k in s.get("nan", ()):
        v[k] = torch.full(shape, float("nan"))
    return dict(v, eu=eu, et=et, coef=torch.tensor(ROW[s["row"]], dtype=torch.float32),
                gs=s.get("gs", 7.5), gr=s.get("gr", 0.0))


def dpm2_update(x, eu, et, z, S, coef, gs, gr, depth=None):
    """x, eu, et (or None), z, S fp32 [batch, n]; coef fp32 (p, q, h, c, second); gs, gr as the C ABI passes them ->
    dict(out, e_out, d, E, second) float64 [batch, n]; stage 1: the new S is x itself"""
    p, q, h, c, second = coef.double().tolist()
    E, e_E = guided(eu, et, gs, gr, depth)
    qE = abs(q) * (E.abs() + e_E)
    if p != 0.0:
        px = p * x.double()
        d = px + q * E
        e_d = abs(q) * e_E + 1.01 * U32 * 2 * (px.abs() + qE)
    else:
        d = q * E
        e_d = abs(q) * e_E + 1.01 * U32 * qE
    base = (S if second != 0.0 else x).double()
    hd = abs(h) * (d.abs() + e_d)
    out = base + h * d
    if second != 0.0 and c != 0.0:
        cz = c * z.double()
        out = out + cz
        e_out = abs(h) * e_d + 1.01 * U32 * (2 * base.abs() + 3 * hd + 2 * cz.abs())
    else:
        e_out = abs(h) * e_d + 1.01 * U32 * (base.abs() + 2 * hd)
    return dict(out=out, e_out=e_out, d=d, E=E, second=second != 0.0)


def ratios(v, out, S):
    """worst |got - ref| / bound of a case's inputs (inputs()) over every element -> dict(out, S_off): `out` against its bound; the
    number of elements of S that are not x's bits (stage 1) or not the bits S held (stage 2)"""
    r = dpm2_update(v["x"], v["eu"], v["et"], v["z"], v["S"], v["coef"], v["gs"], v["gr"])
    shape = v["x"].shape
    same = lambda a, b: int((a.reshape(shape).view(torch.int32) != b.view(torch.int32)).sum().item())  # noqa: E731
    return {"out": check(out.reshape(shape), r["out"], r["e_out"]), "S_off": same(S, v["S"] if r["second"] else v["x"])}


def accumulated(xs, Ss, zs, outs, coef64, gs, gr, cfg=True, sigma0=1.0):
    """The bound on |fused latents - float64 generic latents| after every launch of a loop whose model outputs and noise were replayed.
    xs[i]: the fused loop's fp32 latents [B, ...] before launch i; Ss[i]: its parked sample before launch i (anything where the row
    does not read it); zs[i]: the fp32 noise plane of launch i (None: a loop without noise); outs[i]: its fp32 model output
    ([2 B, ...] = [uncond, text] with cfg); coef64: (p, q, h, c, second) per launch as Python floats -> list of float64 bounds shaped
    like the latents"""
    E_x = (U32 * xs[0].double().abs() if sigma0 != 1.0 else torch.zeros_like(xs[0], dtype=torch.float64)).flatten(1)
    E_S = torch.zeros_like(E_x)
    res = []
    for x, S, z, o, c64 in zip(xs, Ss, zs, outs, coef64):
        Bn = x.shape[0]
        c32 = torch.tensor(c64, dtype=torch.float32)
        xf = x.flatten(1)
        second, noisy = c64[4] != 0.0, c64[4] != 0.0 and c64[3] != 0.0
        zf = z.flatten(1) if noisy else xf            # (a row that reads no noise)
        r = dpm2_update(xf, o[:Bn].flatten(1), o[Bn:].flatten(1) if cfg else None, zf, S.flatten(1) if second else xf, c32, gs,
                        gr if cfg else 0.0)
        p, q, h, c, _ = c64
        dp, dq, dh, dc, _ = (abs(a - b) for a, b in zip(c32.double().tolist(), c64))
        dd = abs(p) * E_x + dp * xf.double().abs() + dq * r["E"].abs()
        store = 2 * U32 * r["out"].abs() + r["e_out"]
        if not second:
            E_S, E_x = E_x, E_x + abs(h) * dd + dh * r["d"].abs() + store
        else:
            E_x = E_S + abs(h) * dd + dh * r["d"].abs() + (dc * zf.double().abs() if noisy else 0.0) + store
        res.append(E_x.reshape(x.shape))
    return res
