"""Float64 reference and elementwise bound for mi355x_sd_plms_update (csrc/step_tail.hip PlmsStep): one model evaluation of PLMS
sampling -- guidance combine, guidance rescale, the history combination, _get_prev_sample, the ring of stored outputs and the parked
sample -- in one launch. A sibling of tests/heun_bounds.py: the guided model output (guided(): E and its bound e_E) comes from
tests/multistep_bounds.py, check() and U32 from tests/rowmap_bounds.py: |out - ref| <= 2 u |ref| + e for an fp32 store, u = 2^-24, over
EVERY element of out and of the written ring plane; the parked sample and every plane the launch must not write are compared as bits.

What the kernel computes per element, in this order (coef = (a, b, p, q, w0, w1, w2, w3, slot, park, from_park, 0) fp32; P the parked
sample; h1 / h2 / h3 the ring planes slot - 1 / slot - 2 / slot - 3 mod 3, the last one the plane `slot` itself):
    E   = the guided (and rescaled) model output                    e_E of multistep_bounds.guided
    m   = fl(w0 E), then m = fl(m + fl(w_k h_k)) for k = 1, 2, 3    only where w_k != 0: h_k does not enter otherwise
    S   = P if from_park else x                                     the other one does not enter
    m'  = fl(fl(p S) + fl(q m))                                     only where p != 0; p == 0: m' = m
    out = fl(fl(a S) + fl(b m'))
    plane[slot] <- E unless from_park;  P <- x (bit copy) where park
(which products fuse into the sums is the compiler's choice: a fused product drops one rounding, the bound covers both).

The bound (1.01 absorbs second-order products of u terms, as in guidance_bounds). x, P and the planes are read, E is computed (e_E):
  * m: K terms are formed (K = 1 + the number of non-zero w_1..3). A term passes its product and at most K - 1 sums, so every term
    passes at most K roundings, each on a partial sum no larger than the ABSOLUTE sum of the terms:
        A   = |w0| (|E| + e_E) + sum |w_k h_k|,     e_m = |w0| e_E + 1.01 u K A.
    The absolute sum is what the bound must carry: the four-term row has weights (55, -59, 37, -9) / 24, of absolute sum 160 / 24
    against a net 1, so on a smooth history the roundings are 6.7 times what the size of m suggests.
  * m' (p != 0): p S and q m pass their product and the sum (2 roundings each):
        e_m' = |q| e_m + 1.01 u 2 (|p S| + |q| (|m| + e_m));    p == 0: e_m' = e_m.
  * out: a S and b m' pass their product and the sum (2 each):
        e_out = |b| e_m' + 1.01 u 2 (|a S| + |b| (|m'| + e_m')).
  * the written plane is E itself: |plane - E| <= 2 u |E| + e_E (check's store term).  P is a copy: it must equal x bit for bit.
The reference of a row reads only what that row may read: a term formed with a zero weight over a NaN plane, an S taken from the
wrong one of x and P, a conversion taken with x on the row that starts from P, two planes exchanged, a dropped term, e stored after
its conversion, or e stored on the row that must store nothing all leave the bound (tests/test_plms_bounds.py injects them).

accumulated() carries the bound through a loop against the generic loop (scheduler.step) run in float64 on the model outputs the fused
loop saw. Errors travel in x (E_x), in the parked sample (E_P) and in the three planes (E_H[k]): the generic loop's history is the
float64 E, the ring holds its fp32 store. With c the float64 row, c32 its fp32 table entry, ref the kernel's float64 value at the
fused inputs:
    E_H[slot]' = 2 u |E| + e_E                                                            (unless from_park)
    dm   = |w32_0 - w_0| |E| + sum_k (|w_k| E_H[plane k] + |w32_k - w_k| |h_k|)          (the planes BEFORE this launch's store)
    E_S  = E_P if from_park else E_x
    dm'  = |p| E_S + |p32 - p| |S| + |q| dm + |q32 - q| |m|                                (p == 0: dm' = dm)
    E_x' = |a| E_S + |a32 - a| |S| + |b| dm' + |b32 - b| |m'| + (2 u |ref| + e_out),      E_P' = E_x where park
E_0 = u |x_0| if the start was scaled by init_noise_sigma != 1 (PNDM: 1). The float64 roundings of the generic loop's own formulas
are 2^-29 of these and are not counted, as in the sibling modules.
"""
import torch

from paddlemix_amd.schedulers import PNDMScheduler
from tests.guidance_bounds import RESIDENT
from tests.multistep_bounds import guided
from tests.rowmap_bounds import U32, check
from tests.step_pieces import base_inputs

SCHED = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", skip_prk_steps=True, steps_offset=1)
WIDTH = 12   # fp32 values in a row


def schedule_rows(steps=20, **kw):
    """the 12 values of every model evaluation of a schedule (steps + 1 rows), as Python floats"""
    sch = PNDMScheduler(**dict(SCHED, **kw))
    sch.set_timesteps(steps)
    with sch.coefficient_walk():
        return [sch.plms_coefficients(t) for t in sch.timesteps]


ROWS_V, ROWS_EPS = schedule_rows(prediction_type="v_prediction"), schedule_rows()
# counter 0 .. 6 of either prediction type: 0 parks, 1 averages from the parked sample, 2 / 3 the shorter histories, 4 the first
# four-term row and the first WRAP (slot 0 again, over three live planes), 5 / 6 the slots 1 and 2 with every plane live
ROW = {**{f"v{c}": ROWS_V[c] for c in range(7)}, **{f"eps{c}": ROWS_EPS[c] for c in range(7)}, "last": ROWS_V[-1]}
POINTERS = ("x", "eu", "et", "P", "H", "out")
_ALL = tuple(f"{k}{c}" for k in ("v", "eps") for c in range(5))
_SOME = ("v0", "v1", "v4")
CASES = {   # name: batch, per_sample and what differs from gs = 7.5, gr = 0, CFG, random inputs and state, aligned pointers
    **{f"b2 n512 vectors {r}": dict(batch=2, n=512, row=r) for r in _ALL + ("v5", "v6", "last")},
    **{f"b1 n251 scalar, unaligned planes {r}": dict(batch=1, n=251, row=r) for r in ("v0", "v1", "v2", "v3", "v4", "eps4", "v5")},
    **{f"b1 n1 {r}": dict(batch=1, n=1, row=r) for r in _SOME},
    **{f"b2 n512 no eps_text {r}": dict(batch=2, n=512, row=r, cfg=False) for r in _SOME + ("eps3",)},
    "b1 n251 no eps_text v4": dict(batch=1, n=251, row="v4", cfg=False),
    **{f"b2 n512 {p} offset one element {r}": dict(batch=2, n=512, row=r, misalign=p) for p in POINTERS for r in _SOME},
    **{f"b2 n512 out=x {r}": dict(batch=2, n=512, row=r, alias=True) for r in _SOME + ("eps2",)},
    **{f"{b} c0 NaN park and ring": dict(batch=2, n=n, row="v0", nan=("P", "h1", "h2", "h3"), **kw)
       for b, n, kw in (("b2 n512", 512, {}), ("b2 n251", 251, {}), ("b2 n1024 rescale", 1024, dict(gr=0.7)))},
    **{f"{b} c1 NaN x, h2 and h3": dict(batch=2, n=n, row="v1", nan=("x", "h2", "h3"), **kw)
       for b, n, kw in (("b2 n512", 512, {}), ("b2 n251", 251, {}), ("b2 n1024 rescale", 1024, dict(gr=0.7)))},
    **{f"{b} c2 NaN h2, h3 and park": dict(batch=2, n=n, row="v2", nan=("h2", "h3", "P"), **kw)
       for b, n, kw in (("b2 n512", 512, {}), ("b2 n251", 251, {}), ("b2 n1024 rescale", 1024, dict(gr=0.7)))},
    "b2 n512 c3 NaN h3 and park": dict(batch=2, n=512, row="eps3", nan=("h3", "P")),
    "b2 n512 c4 NaN park": dict(batch=2, n=512, row="eps4", nan=("P",)),
    **{f"b2 n1024 rescale {r}": dict(batch=2, n=1024, gr=0.7, row=r) for r in ("v0", "v1", "v2", "v3", "v4", "eps4", "v6")},
    **{f"b1 n2 smallest rescale {r}": dict(batch=1, n=2, gr=0.7, row=r) for r in _SOME},
    **{f"b3 n1023 odd rescale {r}": dict(batch=3, n=1023, gr=0.7, row=r) for r in _SOME},
    **{f"b2 n1024 rescale offset 64 {r}": dict(batch=2, n=1024, gr=0.7, row=r, kind="offset") for r in ("v1", "v4")},
    "b2 n1024 rescale out=x v4": dict(batch=2, n=1024, gr=0.7, row="v4", alias=True),
    "b2 n32768 rescale resident v4": dict(batch=2, n=RESIDENT, gr=0.7, row="v4"),
    **{f"b2 n32772 rescale loop form {r}": dict(batch=2, n=RESIDENT + 4, gr=0.7, row=r) for r in _SOME},
    "b2 n32772 rescale loop form c0 NaN park and ring": dict(batch=2, n=RESIDENT + 4, gr=0.7, row="v0", nan=("P", "h1", "h2", "h3")),
}


def flags(coef):
    """(slot, park, from_park) of a row as the kernel takes them"""
    s = float(coef[8])
    from_park = float(coef[10]) != 0.0
    return (2 if s >= 1.5 else 1 if s >= 0.5 else 0), (float(coef[9]) != 0.0 and not from_park), from_park


def inputs(name):
    """dict(x, eu, et (None: no guidance), P, H [3, batch, n], coef, gs, gr) of a case: CPU fp32, seeded by the name"""
    s = CASES[name]
    g, shape, x, eu, et = base_inputs(name, s)
    # P is NOT near x, and the planes are unrelated: an S from the wrong one, or two planes exchanged, shows
    P, H = 3.0 * torch.randn(shape, generator=g), torch.randn((3,) + shape, generator=g)
    coef = torch.tensor(ROW[s["row"]], dtype=torch.float32)
    slot = flags(coef)[0]
    for k in s.get("nan", ()):
        if k == "x":
            x = torch.full(shape, float("nan"))
        elif k == "P":
            P = torch.full(shape, float("nan"))
        else:
            H[(slot - int(k[1])) % 3] = float("nan")
    return dict(x=x, eu=eu, et=et, P=P, H=H, coef=coef, gs=s.get("gs", 7.5), gr=s.get("gr", 0.0))


def plms_update(x, eu, et, P, H, coef, gs, gr, depth=None):
    """x, eu, et (or None), P fp32 [batch, n]; H fp32 [3, batch, n]; coef fp32, 12 values; gs, gr as the C ABI passes them ->
    dict(out, e_out, E, e_E, m, mc, S, hs) float64: m the combination, mc the converted one, hs the planes h1, h2, h3 (None: not read)"""
    a, b, p, q, w0, w1, w2, w3 = coef.double().tolist()[:8]
    slot, _, from_park = flags(coef)
    E, e_E = guided(eu, et, gs, gr, depth)
    hs = [H[(slot - k) % 3].double() if w != 0.0 else None for k, w in ((1, w1), (2, w2), (3, w3))]
    m = w0 * E
    A = abs(w0) * (E.abs() + e_E)
    K = 1
    for w, h in zip((w1, w2, w3), hs):
        if h is not None:
            m = m + w * h
            A = A + (w * h).abs()
            K += 1
    e_m = abs(w0) * e_E + 1.01 * U32 * K * A
    S = (P if from_park else x).double()
    if p != 0.0:
        mc = p * S + q * m
        e_mc = abs(q) * e_m + 1.01 * U32 * 2 * ((p * S).abs() + abs(q) * (m.abs() + e_m))
    else:
        mc, e_mc = m, e_m
    out = a * S + b * mc
    e_out = abs(b) * e_mc + 1.01 * U32 * 2 * ((a * S).abs() + abs(b) * (mc.abs() + e_mc))
    return dict(out=out, e_out=e_out, E=E, e_E=e_E, m=m, mc=mc, S=S, hs=hs)


def ratios(v, out, P, H):
    """worst |got - ref| / bound of a case's inputs (inputs()) over every element -> dict(out, hist, state_off): `out` against its
    bound; the plane the launch writes against E (0.0 where the row writes none); the number of elements of the parked sample and of
    the planes the launch must not write whose bits are not what they must be (P: x's where the row parks, else the ones it held)"""
    r = plms_update(v["x"], v["eu"], v["et"], v["P"], v["H"], v["coef"], v["gs"], v["gr"])
    shape = v["x"].shape
    slot, park, from_park = flags(v["coef"])
    same = lambda a, b: int((a.reshape(shape).view(torch.int32) != b.view(torch.int32)).sum().item())  # noqa: E731
    H = H.reshape((3,) + tuple(shape))
    res = {"out": check(out.reshape(shape), r["out"], r["e_out"]), "hist": 0.0, "state_off": same(P, v["x"] if park else v["P"])}
    for k in range(3):
        if k == slot and not from_park:
            res["hist"] = check(H[k], r["E"], r["e_E"])
        else:
            res["state_off"] += same(H[k], v["H"][k])
    return res


def accumulated(xs, states, outs, coef64, gs, gr, cfg=True, sigma0=1.0):
    """The bound on |fused latents - float64 generic latents| after every launch of a loop whose model outputs were replayed.
    xs[i]: the fused loop's fp32 latents [B, ...] before launch i; states[i]: (P, H), its parked sample and ring [3, B, ...] before
    launch i (anything where the row does not read them); outs[i]: its fp32 model output ([2 B, ...] = [uncond, text] with cfg);
    coef64: the 12 values per launch as Python floats -> list of float64 bounds shaped like the latents"""
    E_x = (U32 * xs[0].double().abs() if sigma0 != 1.0 else torch.zeros_like(xs[0], dtype=torch.float64)).flatten(1)
    E_P, E_H = torch.zeros_like(E_x), [torch.zeros_like(E_x) for _ in range(3)]
    res = []
    for x, (P, H), o, c64 in zip(xs, states, outs, coef64):
        Bn = x.shape[0]
        c32 = torch.tensor(c64, dtype=torch.float32)
        assert c32[8:].tolist() == list(c64[8:])
        slot, park, from_park = flags(c32)
        r = plms_update(x.flatten(1), o[:Bn].flatten(1), o[Bn:].flatten(1) if cfg else None, P.flatten(1), H.flatten(2), c32, gs,
                        gr if cfg else 0.0)
        a, b, p, q, w0 = c64[:5]
        da, db, dp, dq, dw0, dw1, dw2, dw3 = (abs(u - v) for u, v in zip(c32.double().tolist()[:8], c64[:8]))
        dm = dw0 * r["E"].abs()
        for k, (w, dw, h) in enumerate(zip(c64[5:8], (dw1, dw2, dw3), r["hs"]), start=1):
            if h is not None:
                dm = dm + abs(w) * E_H[(slot - k) % 3] + dw * h.abs()
        E_S = E_P if from_park else E_x
        if p != 0.0:
            dm = abs(p) * E_S + dp * r["S"].abs() + abs(q) * dm + dq * r["m"].abs()
        if park:
            E_P = E_x
        if not from_park:
            E_H[slot] = 2 * U32 * r["E"].abs() + r["e_E"]
        E_x = abs(a) * E_S + da * r["S"].abs() + abs(b) * dm + db * r["mc"].abs() + 2 * U32 * r["out"].abs() + r["e_out"]
        res.append(E_x.reshape(x.shape))
    return res
