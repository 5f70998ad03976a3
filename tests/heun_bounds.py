"""Float64 reference and elementwise bound for mi355x_sd_heun_update (csrc/step_tail.hip HeunStep): one model evaluation of a
two-stage Heun step -- guidance combine, guidance rescale, the derivative, the update and the parked state -- in one launch. A sibling
of tests/ancestral_bounds.py: the guided model output (guided(): E and its bound e_E) comes from tests/multistep_bounds.py, check()
and U32 from tests/rowmap_bounds.py: |out - ref| <= 2 u |ref| + e for an fp32 store, u = 2^-24, over EVERY element of out, S and D.

What the kernel computes per element, in this order (coef = (p, q, h, g, second) fp32, S / D the parked sample / derivative):
    E   = the guided (and rescaled) model output                    e_E of multistep_bounds.guided
    d   = fl(fl(p x) + fl(q E))                                     p == 0: d = fl(q E), x does not enter
    second == 0:  out = fl(x + fl(h d))      S <- x (bit copy)   D <- d            S and D are NOT read
    second != 0:  m   = fl(fl(g D) + d)      g == 0: m = d and D is NOT read; g == 1: fl(g D) = D exactly
                  out = fl(S + fl(h m))      S and D are NOT written
(which products fuse into the sums is the compiler's choice: a fused product drops one rounding, the bound covers both).

The bound (1.01 absorbs second-order products of u terms, as in guidance_bounds). x, S and D are read, E is computed (e_E):
  * d: the computed E enters through q. p != 0: p x and q E pass their product and the sum (2 roundings each); p == 0: q E passes its
    product alone (1):
        e_d = |q| e_E + 1.01 u r_d (|p x| + |q| (|E| + e_E)),  r_d = 2 (p != 0) or 1 (p == 0).            This is D's bound in stage 1.
  * stage 1: x passes the sum (1), h d its product and the sum (2):
        e_out = |h| e_d + 1.01 u (|x| + 2 |h| (|d| + e_d)).     S is a copy: it must equal x bit for bit (its bound is 0).
  * stage 2: g D passes its product and the sum (2; at g == 1 the product is exact: 1), d passes the sum (1):
        e_m   = e_d + 1.01 u (r_g |g D| + |d| + e_d),  r_g = 1 (g == 1) or 2;     g == 0: m = d, e_m = e_d, and D does not appear
        e_out = |h| e_m + 1.01 u (|S| + 2 |h| (|m| + e_m)).
    x does not appear in stage 2 but through d. The reference of a stage reads only what that stage may read: a stage 1 that forms a
    term over a NaN S or D, or a stage 2 at g == 0 that forms 0 * D over a NaN plane, leaves the bound (inf); a stage 2 that starts
    from x instead of S is off by |x - S|; a D rounded to 8 mantissa bits before use by |h g D| 2^-9 against u |h g D|
    (tests/test_heun_bounds.py injects all of them).

accumulated() carries the bound through a loop against the generic loop (scheduler.step) run in float64 on the model outputs the fused
loop saw. Three errors travel: E_x of the latents, E_S of the parked sample, E_D of the parked derivative. With (p, q, h, g) the float64
coefficients, x32 the fp32 table entries, x_i / S_i / D_i the fused loop's buffers, ref the kernel's float64 value at the fused inputs:
    dd   = |p| E_x + |p32 - p| |x_i| + |q32 - q| |E|                                      (ref d against the generic derivative)
    stage 1:  E_x' = E_x + |h| dd + |h32 - h| |d| + (2 u |ref| + e_out),   E_S' = E_x,   E_D' = dd + 2 u |d| + e_d
    stage 2:  dm   = |g| E_D + dd
              E_x' = E_S + |h| dm + |h32 - h| |m| + (2 u |ref| + e_out)                    (g is 0 or 1: g32 = g)
E_0 = u |x_0| if the start was scaled by init_noise_sigma != 1 (one fp32 product). The float64 roundings of the generic loop's own
formulas (x0, (x - x0) / sigma, the average) are 2^-29 of these and are not counted, as in the sibling modules.
"""
import torch

from paddlemix_amd.schedulers import HeunDiscreteScheduler
from tests.guidance_bounds import RESIDENT
from tests.multistep_bounds import guided
from tests.rowmap_bounds import U32, check
from tests.step_pieces import base_inputs

SCHED = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def schedule_rows(steps=20, **kw):
    """(p, q, h, g, second) of every model evaluation of a schedule (2 * steps - 1 rows), as Python floats"""
    sch = HeunDiscreteScheduler(**dict(SCHED, **kw))
    sch.set_timesteps(steps)
    with sch.coefficient_walk():
        return [sch.heun_coefficients(t) for t in sch.timesteps]


ROWS_V, ROWS_EPS = schedule_rows(prediction_type="v_prediction"), schedule_rows()
ROW = {"v1": ROWS_V[10], "v2": ROWS_V[11], "eps1": ROWS_EPS[10], "eps2": ROWS_EPS[11], "last": ROWS_V[-1],
       "g0": ROWS_V[11][:3] + (0.0, 1.0)}   # stage 1 / stage 2 with p != 0; with p == 0; the last row (stage 1 to sigma = 0); stage 2 at g == 0
POINTERS = ("x", "eu", "et", "S", "D", "out")
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
    **{f"b2 n512 no eps_text {s}": dict(batch=2, n=512, row=r, cfg=False) for s, r in _BOTH},
    "b1 n251 no eps_text stage 1": dict(batch=1, n=251, row="v1", cfg=False),
    **{f"b2 n512 {p} offset one element {s}": dict(batch=2, n=512, row=r, misalign=p) for p in POINTERS for s, r in _BOTH},
    **{f"b2 n512 out=x {s}": dict(batch=2, n=512, row=r, alias=True) for s, r in _BOTH},
    "b2 n512 stage 1 NaN state": dict(batch=2, n=512, row="v1", nan=("S", "D")),
    "b1 n251 stage 1 NaN state": dict(batch=1, n=251, row="eps1", nan=("S", "D")),
    "b2 n512 stage 2 g0 NaN D": dict(batch=2, n=512, row="g0", nan=("D",)),
    "b1 n251 stage 2 g0 NaN D": dict(batch=1, n=251, row="g0", nan=("D",)),
    **{f"b2 n1024 rescale {s}": dict(batch=2, n=1024, gr=0.7, row=r) for s, r in _BOTH},
    **{f"b1 n2 smallest rescale {s}": dict(batch=1, n=2, gr=0.7, row=r) for s, r in _BOTH},
    **{f"b3 n1023 odd rescale {s}": dict(batch=3, n=1023, gr=0.7, row=r) for s, r in _BOTH},
    **{f"b2 n1024 rescale offset 64 {s}": dict(batch=2, n=1024, gr=0.7, row=r, kind="offset") for s, r in _BOTH},
    "b2 n1024 rescale out=x stage 1": dict(batch=2, n=1024, gr=0.7, row="v1", alias=True),
    "b2 n1024 rescale epsilon row stage 2": dict(batch=2, n=1024, gr=0.7, row="eps2"),
    "b2 n1024 rescale stage 1 NaN state": dict(batch=2, n=1024, gr=0.7, row="v1", nan=("S", "D")),
    "b2 n1024 rescale stage 2 g0 NaN D": dict(batch=2, n=1024, gr=0.7, row="g0", nan=("D",)),
    **{f"b2 n32768 rescale resident {s}": dict(batch=2, n=RESIDENT, gr=0.7, row=r) for s, r in _BOTH},
    **{f"b2 n32772 rescale loop form {s}": dict(batch=2, n=RESIDENT + 4, gr=0.7, row=r) for s, r in _BOTH},
    "b2 n32772 rescale loop form stage 1 NaN state": dict(batch=2, n=RESIDENT + 4, gr=0.7, row="v1", nan=("S", "D")),
}


def inputs(name):
    """dict(x, eu, et (None: no guidance), S, D, coef, gs, gr) of a case: CPU fp32 [batch, n], seeded by the name"""
    s = CASES[name]
    g, shape, x, eu, et = base_inputs(name, s)
    S, D = 3.0 * torch.randn(shape, generator=g), torch.randn(shape, generator=g)   # S is NOT near x: a stage 2 from x shows
    nan = s.get("nan", ())
    S = torch.full(shape, float("nan")) if "S" in nan else S
    D = torch.full(shape, float("nan")) if "D" in nan else D
    return dict(x=x, eu=eu, et=et, S=S, D=D, coef=torch.tensor(ROW[s["row"]], dtype=torch.float32),
                gs=s.get("gs", 7.5), gr=s.get("gr", 0.0))


def heun_update(x, eu, et, S, D, coef, gs, gr, depth=None):
    """x, eu, et (or None), S, D fp32 [batch, n]; coef fp32 (p, q, h, g, second); gs, gr as the C ABI passes them ->
    dict(out, e_out, d, e_d, m, E, second) float64 [batch, n]; stage 1: the new S is x itself and the new D is d within e_d"""
    p, q, h, g, second = coef.double().tolist()
    E, e_E = guided(eu, et, gs, gr, depth)
    qE = abs(q) * (E.abs() + e_E)
    if p != 0.0:
        px = p * x.double()
        d = px + q * E
        e_d = abs(q) * e_E + 1.01 * U32 * 2 * (px.abs() + qE)
    else:
        d = q * E
        e_d = abs(q) * e_E + 1.01 * U32 * qE
    if second == 0.0:
        m = d
        out = x.double() + h * d
        e_out = abs(h) * e_d + 1.01 * U32 * (x.double().abs() + 2 * abs(h) * (d.abs() + e_d))
    else:
        if g != 0.0:
            gD = g * D.double()
            m = gD + d
            e_m = e_d + 1.01 * U32 * ((1 if g == 1.0 else 2) * gD.abs() + d.abs() + e_d)
        else:
            m, e_m = d, e_d
        out = S.double() + h * m
        e_out = abs(h) * e_m + 1.01 * U32 * (S.double().abs() + 2 * abs(h) * (m.abs() + e_m))
    return dict(out=out, e_out=e_out, d=d, e_d=e_d, m=m, E=E, second=second != 0.0)


def ratios(v, out, S, D):
    """worst |got - ref| / bound of a case's inputs (inputs()) over every element -> dict(out, D, S_off): `out` against its bound; in
    stage 1 the written D against e_d and the number of elements of the written S that are not x's bits; in stage 2 the number of
    elements of S and D that are not the bits they held (D ratio 0.0)"""
    r = heun_update(v["x"], v["eu"], v["et"], v["S"], v["D"], v["coef"], v["gs"], v["gr"])
    shape = v["x"].shape
    same = lambda a, b: int((a.reshape(shape).view(torch.int32) != b.view(torch.int32)).sum().item())  # noqa: E731
    res = {"out": check(out.reshape(shape), r["out"], r["e_out"])}
    if r["second"]:
        res["D"], res["S_off"] = 0.0, same(S, v["S"]) + same(D, v["D"])
    else:
        res["D"], res["S_off"] = check(D.reshape(shape), r["d"], r["e_d"]), same(S, v["x"])
    return res


def accumulated(xs, states, outs, coef64, gs, gr, cfg=True, sigma0=1.0):
    """The bound on |fused latents - float64 generic latents| after every launch of a loop whose model outputs were replayed.
    xs[i]: the fused loop's fp32 latents [B, ...] before launch i; states[i]: (S, D), its parked planes before launch i (anything
    where the stage does not read them); outs[i]: its fp32 model output ([2 B, ...] = [uncond, text] with cfg); coef64:
    (p, q, h, g, second) per launch as Python floats -> list of float64 bounds shaped like the latents"""
    E_x = (U32 * xs[0].double().abs() if sigma0 != 1.0 else torch.zeros_like(xs[0], dtype=torch.float64)).flatten(1)
    E_S, E_D = torch.zeros_like(E_x), torch.zeros_like(E_x)
    res = []
    for x, (S, D), o, c64 in zip(xs, states, outs, coef64):
        Bn = x.shape[0]
        c32 = torch.tensor(c64, dtype=torch.float32)
        xf = x.flatten(1)
        second = c64[4] != 0.0
        Sf, Df = (S.flatten(1), D.flatten(1)) if second else (xf, xf)   # (stage 1 reads neither)
        r = heun_update(xf, o[:Bn].flatten(1), o[Bn:].flatten(1) if cfg else None, Sf, Df, c32, gs, gr if cfg else 0.0)
        p, q, h, g, _ = c64
        dp, dq, dh, dg, _ = (abs(a - b) for a, b in zip(c32.double().tolist(), c64))
        assert dg == 0.0
        dd = abs(p) * E_x + dp * xf.double().abs() + dq * r["E"].abs()
        store = 2 * U32 * r["out"].abs() + r["e_out"]
        if not second:
            E_S, E_D = E_x, dd + 2 * U32 * r["d"].abs() + r["e_d"]
            E_x = E_x + abs(h) * dd + dh * r["d"].abs() + store
        else:
            E_x = E_S + abs(h) * (abs(g) * E_D + dd) + dh * r["m"].abs() + store
        res.append(E_x.reshape(x.shape))
    return res
