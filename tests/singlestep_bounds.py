"""Float64 reference and elementwise bound for mi355x_sd_singlestep_update (csrc/step_tail.hip SinglestepStep): one model evaluation of
DPM-Solver singlestep sampling -- guidance combine, guidance rescale, convert_model_output, the update, the parked sample and the
group's converted outputs -- in one launch. A sibling of tests/plms_bounds.py: the guided model output (guided(): E and its bound e_E)
comes from tests/multistep_bounds.py, check() and U32 from tests/rowmap_bounds.py: |out - ref| <= 2 u |ref| + e for an fp32 store,
u = 2^-24, over EVERY element of out and of the written plane; the parked sample and every plane the launch must not write are
compared as bits.

What the kernel computes per element, in this order (coef = (p, q, A, B, E1, E2, order, keep) fp32; S the parked sample; b / m1 the
planes 0 / 1 of hist):
    E   = the guided (and rescaled) model output                           e_E of multistep_bounds.guided
    m0  = fl(fl(p x) + fl(q E))
    order 1:  out = fl(fl(A x) + fl(B m0))                                 S <- x (bit copy), plane 0 <- m0; S and hist do not enter
    order 2:  out = fl(fl(fl(A S) + fl(B b)) + fl(E1 fl(m0 - b)))          plane 1 <- m0 where keep != 0; plane 1 does not enter
    order 3:  the same, then out = fl(out + fl(E2 fl(m1 - b)))             only where E2 != 0: plane 1 does not enter otherwise
(which products fuse into the sums is the compiler's choice: a fused product drops one rounding, the bound covers both).

The bound (1.01 absorbs second-order products of u terms, as in guidance_bounds). x, S, b and m1 are read, E is computed (e_E):
  * m0, two products and a sum of a read value and a computed one, as in multistep_bounds:
        e_m0 = |q| e_E + 1.01 u 2 (|p x| + |q| (|E| + e_E)).      This is also the written plane's bound (plus check's store term).
    At p == 0 and q == 1 (epsilon prediction under "dpmsolver", sample prediction under "dpmsolver++") both products and the sum are
    exact, m0 is E itself and e_m0 = e_E: without guidance m0 is then a value the launch READ, and carries no error at all.
  * order 1: A x and B m0 pass their product and the sum (2 roundings each):
        e_out = |B| e_m0 + 1.01 u 2 (|A x| + |B| (|m0| + e_m0)).
  * orders 2 and 3, K terms (3, or 4 with E2 != 0) summed left to right. A S and B b pass their product and K - 1 sums; a
    difference term passes its difference, its product and at most K - 2 sums: no term passes more than K roundings. The computed
    m0 enters through E1 alone, inside a difference whose other operand is read:
        e_out = |E1| e_m0 + 1.01 u K (|A S| + |B b| + |E1| (|m0 - b| + e_m0) + |E2| |m1 - b|).
    The regrouped (B - E1 - E2) b + E1 m0 + E2 m1 would carry u (|B - E1 - E2| |b| + |E1| |m0| + |E2| |m1|) instead of
    u (|E1| |m0 - b| + |E2| |m1 - b|): E1 and E2 carry 1 / r0, 1 / r1 and 1 / (r0 - r1), the group's outputs are close to each other,
    and the form leaves the bound (tests/test_singlestep_bounds.py injects it, with a form that reads the parked sample at order 1,
    one that parks at order 2 and one that skips the plane-1 store).
The reference of a row reads only what that row may read, and inputs() fills EVERYTHING ELSE of the state with NaN on every case: S
and both planes at order 1, plane 1 at order 2 and at order 3 with E2 == 0.

accumulated() carries the bound through a loop against the generic loop (scheduler.step) run in float64 on the model outputs the fused
loop saw. Errors travel in x (E_x), in the parked sample (E_P) and in the two planes (E_H0, E_H1). With c the float64 row, c32 its
fp32 table entry, ref the kernel's float64 value at the fused inputs, store = 2 u |ref| + e_out:
    dm0  = |p| E_x + |p32 - p| |x| + |q32 - q| |E|                                       (ref m0 against the generic m0)
    order 1:  E_x' = |A| E_x + |A32 - A| |x| + |B| dm0 + |B32 - B| |m0| + store;  E_P' = E_x;  E_H0' = dm0 + 2 u |m0| + e_m0
    order 2+: E_x' = |A| E_P + |A32 - A| |S| + |B| E_H0 + |B32 - B| |b| + |E1| (dm0 + E_H0) + |E1_32 - E1| |m0 - b|
                     + |E2| (E_H1 + E_H0) + |E2_32 - E2| |m1 - b| + store;        E_H1' = dm0 + 2 u |m0| + e_m0 where keep
E_0 = u |x_0| if the start was scaled by init_noise_sigma != 1 (here: 1). The float64 roundings of the generic loop's own formulas
are 2^-29 of these and are not counted, as in the sibling modules.
"""
import torch

from paddlemix_amd.schedulers import DPMSolverSinglestepScheduler
from tests.guidance_bounds import RESIDENT
from tests.multistep_bounds import guided
from tests.rowmap_bounds import U32, check
from tests.step_pieces import base_inputs, counting

SCHED = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
WIDTH = 8   # fp32 values in a row


def scheduler(**kw):
    """a counted DPMSolverSinglestepScheduler on the SD betas"""
    return counting(DPMSolverSinglestepScheduler(**dict(SCHED, **kw)))


def schedule_rows(steps=20, **kw):
    """the 8 values of every model evaluation of a schedule, as Python floats"""
    sch = DPMSolverSinglestepScheduler(**dict(SCHED, **kw))
    sch.set_timesteps(steps)
    with sch.coefficient_walk():
        return [sch.singlestep_coefficients(t) for t in sch.timesteps]


# v rows: dpmsolver++ with v-prediction (p = alpha_t); eps rows: dpmsolver with epsilon prediction (p = 0, q = 1)
_V, _EPS = dict(prediction_type="v_prediction"), dict(algorithm_type="dpmsolver")
_KINDS = {"o1": (dict(solver_order=3, solver_type="heun"), 9), "o2k1": (dict(solver_order=3, solver_type="heun"), 10),
          "o3h": (dict(solver_order=3, solver_type="heun"), 11), "o3m": (dict(solver_order=3), 11), "o2k0": (dict(), 11)}
ROW = {f"{pt}_{k}": schedule_rows(**kw, **pkw)[i] for pt, pkw in (("v", _V), ("eps", _EPS)) for k, (kw, i) in _KINDS.items()}
KINDS = tuple(_KINDS)
POINTERS = ("x", "eu", "et", "P", "H", "out")
_ALL = tuple(ROW)
_SOME = ("v_o1", "v_o2k1", "v_o3h")
CASES = {   # name: batch, per_sample and what differs from gs = 7.5, gr = 0, CFG, random inputs, aligned pointers
    **{f"b2 n512 vectors {r}": dict(batch=2, n=512, row=r) for r in _ALL},
    **{f"b1 n251 scalar, unaligned planes {r}": dict(batch=1, n=251, row=r) for r in _ALL},
    **{f"b3 n1023 scalar, odd {r}": dict(batch=3, n=1023, row=r) for r in _ALL},
    **{f"b2 n512 no eps_text {r}": dict(batch=2, n=512, row=r, cfg=False) for r in _SOME + ("eps_o2k1", "eps_o3h", "eps_o3m")},
    **{f"b2 n512 {p} offset one element {r}": dict(batch=2, n=512, row=r, misalign=p) for p in POINTERS for r in _SOME},
    **{f"b2 n512 out=x {r}": dict(batch=2, n=512, row=r, alias=True) for r in _SOME + ("eps_o3m", "eps_o2k0")},
    **{f"b2 n1024 rescale {r}": dict(batch=2, n=1024, gr=0.7, row=r) for r in _ALL},
    "b2 n1024 rescale out=x v_o3h": dict(batch=2, n=1024, gr=0.7, row="v_o3h", alias=True),
    **{f"b2 n32772 rescale loop form {r}": dict(batch=2, n=RESIDENT + 4, gr=0.7, row=r) for r in _ALL},
}
WRAPPED = ("b2 n1024 rescale v_o3h", "b2 n512 vectors v_o2k1", "b2 n512 vectors eps_o1")   # also run through ops.singlestep_update


def flags(coef):
    """(order, keep, heun) of a row as the kernel takes them"""
    o = float(coef[6])
    order = 3 if o >= 2.5 else 2 if o >= 1.5 else 1
    return order, order == 2 and float(coef[7]) != 0.0, order == 3 and float(coef[5]) != 0.0


def inputs(name):
    """dict(x, eu, et (None: no guidance), P, H [2, batch, n], coef, gs, gr) of a case: CPU fp32, seeded by the name. The planes a
    row reads hold what a loop would have left there, outputs of the group CLOSE to this evaluation's m0 (1e-2 of it apart: a
    regrouped sum cancels), the parked sample is NOT near x (an update from the wrong one shows), and whatever the row must not
    read is NaN"""
    s = CASES[name]
    g, shape, x, eu, et = base_inputs(name, s)
    coef = torch.tensor(ROW[s["row"]], dtype=torch.float32)
    gs, gr = s.get("gs", 7.5), s.get("gr", 0.0)
    order, _, heun = flags(coef)
    P, near = 3.0 * torch.randn(shape, generator=g), 1e-2 * torch.randn((2,) + shape, generator=g)
    E, _ = guided(eu, et, gs, gr)
    m0 = float(coef[0]) * x.double() + float(coef[1]) * E
    H = (m0 * (1 + near.double())).float()
    nan = float("nan")
    if order == 1:
        P, H = torch.full(shape, nan), torch.full((2,) + shape, nan)
    elif not heun:
        H[1] = nan
    return dict(x=x, eu=eu, et=et, P=P, H=H, coef=coef, gs=gs, gr=gr)


def singlestep_update(x, eu, et, P, H, coef, gs, gr, depth=None):
    """x, eu, et (or None), P fp32 [batch, n]; H fp32 [2, batch, n]; coef fp32, 8 values; gs, gr as the C ABI passes them ->
    dict(out, e_out, E, m0, e_m0, S, b, d0, d1) float64: S the start of the update, b the base, d0 = m0 - b, d1 = m1 - b (zeros where
    the row does not form them)"""
    p, q, A, B, E1, E2 = coef.double().tolist()[:6]
    order, _, heun = flags(coef)
    E, e_E = guided(eu, et, gs, gr, depth)
    px = p * x.double()
    m0 = px + q * E
    e_m0 = e_E if (p, q) == (0.0, 1.0) else abs(q) * e_E + 1.01 * U32 * 2 * (px.abs() + abs(q) * (E.abs() + e_E))
    zero = torch.zeros_like(m0)
    if order == 1:
        S, b, d0, d1 = x.double(), zero, zero, zero
        out = A * S + B * m0
        e_out = abs(B) * e_m0 + 1.01 * U32 * 2 * ((A * S).abs() + abs(B) * (m0.abs() + e_m0))
    else:
        S, b = P.double(), H[0].double()
        d0, d1 = m0 - b, (H[1].double() - b if heun else zero)
        out = A * S + B * b + E1 * d0
        if heun:
            out = out + E2 * d1
        K = 4 if heun else 3
        e_out = abs(E1) * e_m0 + 1.01 * U32 * K * ((A * S).abs() + (B * b).abs() + abs(E1) * (d0.abs() + e_m0) + abs(E2) * d1.abs())
    return dict(out=out, e_out=e_out, E=E, m0=m0, e_m0=e_m0, S=S, b=b, d0=d0, d1=d1)


def ratios(v, out, P, H):
    """worst |got - ref| / bound of a case's inputs (inputs()) over every element -> dict(out, hist, state_off): `out` against its
    bound; the plane the launch writes against m0 (0.0 where the row writes none); the number of elements of the parked sample and of
    the planes the launch must not write whose bits are not what they must be (P: x's at order 1, else the ones it held)"""
    r = singlestep_update(v["x"], v["eu"], v["et"], v["P"], v["H"], v["coef"], v["gs"], v["gr"])
    shape = v["x"].shape
    order, keep, _ = flags(v["coef"])
    same = lambda a, b: int((a.reshape(shape).view(torch.int32) != b.view(torch.int32)).sum().item())  # noqa: E731
    H = H.reshape((2,) + tuple(shape))
    res = {"out": check(out.reshape(shape), r["out"], r["e_out"]), "hist": 0.0, "state_off": same(P, v["x"] if order == 1 else v["P"])}
    written = 0 if order == 1 else 1 if keep else None
    for k in range(2):
        if k == written:
            res["hist"] = check(H[k], r["m0"], r["e_m0"])
        else:
            res["state_off"] += same(H[k], v["H"][k])
    return res


def accumulated(xs, states, outs, coef64, gs, gr, cfg=True, sigma0=1.0):
    """The bound on |fused latents - float64 generic latents| after every launch of a loop whose model outputs were replayed.
    xs[i]: the fused loop's fp32 latents [B, ...] before launch i; states[i]: (P, H), its parked sample and planes [2, B, ...] before
    launch i (anything where the row does not read them); outs[i]: its fp32 model output ([2 B, ...] = [uncond, text] with cfg);
    coef64: the 8 values per launch as Python floats -> list of float64 bounds shaped like the latents"""
    E_x = (U32 * xs[0].double().abs() if sigma0 != 1.0 else torch.zeros_like(xs[0], dtype=torch.float64)).flatten(1)
    E_P, E_H0, E_H1 = torch.zeros_like(E_x), torch.zeros_like(E_x), torch.zeros_like(E_x)
    res = []
    for x, (P, H), o, c64 in zip(xs, states, outs, coef64):
        Bn = x.shape[0]
        c32 = torch.tensor(c64, dtype=torch.float32)
        assert c32[6:].tolist() == list(c64[6:])
        order, keep, heun = flags(c32)
        r = singlestep_update(x.flatten(1), o[:Bn].flatten(1), o[Bn:].flatten(1) if cfg else None, P.flatten(1), H.flatten(2), c32, gs,
                              gr if cfg else 0.0)
        p, q, A, B, E1, E2 = c64[:6]
        dp, dq, dA, dB, dE1, dE2 = (abs(u - v) for u, v in zip(c32.double().tolist()[:6], c64[:6]))
        dm0 = abs(p) * E_x + dp * x.flatten(1).double().abs() + dq * r["E"].abs()
        store = 2 * U32 * r["out"].abs() + r["e_out"]
        plane = dm0 + 2 * U32 * r["m0"].abs() + r["e_m0"]
        if order == 1:
            E_P, E_H0 = E_x, plane
            E_x = abs(A) * E_x + dA * r["S"].abs() + abs(B) * dm0 + dB * r["m0"].abs() + store
        else:
            E_x = abs(A) * E_P + dA * r["S"].abs() + abs(B) * E_H0 + dB * r["b"].abs() + abs(E1) * (dm0 + E_H0) + dE1 * r["d0"].abs() \
                + store
            if heun:
                E_x = E_x + abs(E2) * (E_H1 + E_H0) + dE2 * r["d1"].abs()
            if keep:
                E_H1 = plane
        res.append(E_x.reshape(x.shape))
    return res
