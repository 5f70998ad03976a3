"""Float64 reference and elementwise bound for mi355x_sd_unipc_update (csrc/misc.hip unipc_kernel / unipc_rescale_kernel): one step
of UniPC sampling -- guidance combine, guidance rescale, convert_model_output, the B(h) corrector, the B(h) predictor, last_sample and
the history shift -- in one launch. The sibling of tests/multistep_bounds.py, whose guided() (the bound on the guided and rescaled
model output E) and check() it uses: |got - ref| <= 2 u |ref| + e for an fp32 store, u = 2^-24, over EVERY element of out, last and
history plane 0; planes 1 and 2 are copies and must hold the old planes 0 and 1 bit for bit.

What the kernel computes per element, in this order (coef = (p, q, Ac, Bc, C2, C3, Ct, Ap, Bp, D1, D2, corr) fp32, L = last,
h1 / h2 / h3 = planes 0 / 1 / 2 before the call):
    m_t = fl(fl(p x) + fl(q E))                                                                          -> plane 0
    x_c = fl(fl(fl(fl(fl(Ac L) + fl(Bc h1)) + fl(C2 fl(h2 - h1))) + fl(C3 fl(h3 - h1))) + fl(Ct fl(m_t - h1)))   corr != 0   -> last
    x_c = x                                                                                               corr == 0
    out = fl(fl(fl(fl(Ap x_c) + fl(Bp m_t)) + fl(D1 fl(h1 - m_t))) + fl(D2 fl(h2 - m_t)))
A term whose coefficient is 0.0 is NOT formed: its operand is not read into the arithmetic and the sum has one addition fewer.
Which products fuse into the sums is the compiler's choice: a fused product drops one rounding, the bound covers both.

The bound (1.01 absorbs the second-order products of u terms, as in multistep_bounds):
  * E, e_E: multistep_bounds.guided.
  * m_t: e_mt = |q| e_E + 2 u (|p x| + |q| (|E| + e_E))  -- two products and a sum of a read value and a computed one.
  * a left-to-right sum of N formed terms: term j is rounded by its difference (if it has one), its product and the additions after
    it -- N - 1 for the first two terms, N + 1 - j for term j >= 3 (counting from 1). With r_j that count, t_j the term's exact value
    and i_j the error its computed operand brings in (|Ct| e_mt for the corrector's last term; |Ap| e_xc, |Bp| e_mt, |D_k| e_mt for
    the predictor's),
        e_sum = sum_j ( i_j + 1.01 r_j u (|t_j| + i_j) ).
    L and the planes are read, not computed: they bring no error in. Each term is scaled by ITS OWN magnitude -- |C2| |h2 - h1|, not
    |C2| (|h2| + |h1|): the regrouped C2 h2 - C2 h1 rounds at the latter and leaves the bound when C2 ~ 1 / r_k is large and the planes
    are close (tests/test_unipc_bounds.py injects it).
  * corr == 0: x_c is x itself, e_xc = 0.

accumulated() carries the bound through a loop against the generic loop (scheduler.step) run in float64 on the model outputs the
fused loop saw. Errors travel in the latents (E_x), in last (E_L) and in the planes (E_h[k]). With c64 the float64 coefficients,
c32 the fp32 table row, and ref the kernel's float64 value at the fused loop's own inputs:
    dm   = |p| E_x + |p32 - p| |x| + |q32 - q| |E|                                                  ref m_t against the generic m_t
    dxc  = |Ac| E_L + |dAc| |L| + |Bc| E_h1 + |dBc| |h1| + sum_k (|C_k| (E_hk + E_h1) + |dC_k| |h_k - h1|)
           + |Ct| (dm + E_h1) + |dCt| |m_t - h1|                       corr != 0;   dxc = E_x at corr == 0
    E_x' = |Ap| dxc + |dAp| |x_c| + |Bp| dm + |dBp| |m_t| + sum_k (|D_k| (E_hk + dm) + |dD_k| |h_k - m_t|) + (2 u |out| + e_out)
    E_L' = dxc + (2 u |x_c| + e_xc)   (corr == 0: E_x: last <- x, exactly);   E_h' = [dm + (2 u |m_t| + e_mt), E_h1, E_h2]
Terms with a zero coefficient are skipped here as in the kernel (their E may be anything). E_0 = 0: init_noise_sigma is 1.
"""
import torch

from paddlemix_amd.schedulers import UniPCMultistepScheduler
from tests.guidance_bounds import RESIDENT
from tests.multistep_bounds import SCHED, guided
from tests.rowmap_bounds import U32, check
from tests.step_pieces import base_inputs

NAMES = ("p", "q", "Ac", "Bc", "C2", "C3", "Ct", "Ap", "Bp", "D1", "D2", "corr")


def schedule_rows(steps=10, first=0, **kw):
    """the 12 coefficients of every step run of a schedule, as Python floats"""
    sch = UniPCMultistepScheduler(**dict(SCHED, **kw))
    sch.set_timesteps(steps)
    return [sch.unipc_coefficients(t) for t in sch.timesteps[first:]]


ROWS3 = schedule_rows(solver_order=3)
ROWS2 = schedule_rows()
# order 3: a full step at mid schedule (every coefficient formed), the first step (no corrector, no history), the second (corrector
# of order 1, predictor of order 2); order 2 / order 1 schedulers' mid rows; a row with the corrector disabled
FULL3, FIRST, SECOND = ROWS3[5], ROWS3[0], ROWS3[1]
FULL2 = ROWS2[5]
FULL1 = schedule_rows(solver_order=1)[3]
NOCORR = schedule_rows(disable_corrector=[4])[5]
ROW = {"full3": FULL3, "first": FIRST, "second": SECOND, "full2": FULL2, "full1": FULL1, "nocorr": NOCORR}

CASES = {   # name: batch, per_sample, hist planes and what differs from gs = 7.5, gr = 0.0, row full3, CFG, random inputs
    "b2 n256 o3 vectors": dict(batch=2, n=256, order=3),
    "b2 n255 o3 scalar only": dict(batch=2, n=255, order=3),
    "b2 n255 o1 vectors + tail": dict(batch=2, n=255, order=1, row="full1"),
    "b2 n256 o3 offset 4 bytes": dict(batch=2, n=256, order=3, misalign=True),
    "b2 n256 o2": dict(batch=2, n=256, order=2, row="full2"),
    "b2 n256 o1": dict(batch=2, n=256, order=1, row="full1"),
    "b2 n256 o2 corrector off": dict(batch=2, n=256, order=2, row="nocorr"),
    "b3 n4093 o3 more than one block": dict(batch=3, n=4093, order=3),
    "b2 n256 o3 no eps_text": dict(batch=2, n=256, order=3, cfg=False),
    "b2 n255 o2 no eps_text": dict(batch=2, n=255, order=2, row="full2", cfg=False),
    "b2 n256 o3 rescale": dict(batch=2, n=256, order=3, gr=0.7),
    "b2 n255 o2 rescale": dict(batch=2, n=255, order=2, row="full2", gr=0.7),
    "b1 n2 o1 smallest rescale": dict(batch=1, n=2, order=1, row="full1", gr=0.7),
    "b1 n32768 o3 rescale resident": dict(batch=1, n=RESIDENT, order=3, gr=0.7),
    "b1 n32772 o3 rescale re-reading": dict(batch=1, n=RESIDENT + 4, order=3, gr=0.7),
    "b2 n256 o3 first step NaN state": dict(batch=2, n=256, order=3, row="first", nan_state=True),
    "b2 n255 o3 first step NaN state": dict(batch=2, n=255, order=3, row="first", nan_state=True),
    "b2 n256 o3 rescale first step NaN state": dict(batch=2, n=256, order=3, row="first", nan_state=True, gr=0.7),
    "b2 n256 o3 second step NaN planes 1 2": dict(batch=2, n=256, order=3, row="second", nan_old=True),
    "b2 n256 o3 out=x": dict(batch=2, n=256, order=3, alias=True),
    "b2 n256 o3 rescale out=x": dict(batch=2, n=256, order=3, gr=0.7, alias=True),
    "b1 n32772 o2 rescale out=x": dict(batch=1, n=RESIDENT + 4, order=2, row="full2", gr=0.7, alias=True),
}


def inputs(name):
    """dict(x, eu, et (None: no guidance), last, hist [order, batch, n], coef, gs, gr, order) of a case: CPU fp32, seeded by the name"""
    s = CASES[name]
    g, shape, x, eu, et = base_inputs(name, s)
    last = 3.0 * torch.randn(shape, generator=g)
    hist = 2.0 * torch.randn((s["order"],) + shape, generator=g)
    if s.get("nan_state"):
        last, hist = torch.full_like(last, float("nan")), torch.full_like(hist, float("nan"))
    if s.get("nan_old"):
        hist[1:] = float("nan")
    return dict(x=x, eu=eu, et=et, last=last, hist=hist,
                coef=torch.tensor(ROW[s.get("row", "full3")], dtype=torch.float32), gs=s.get("gs", 7.5), gr=s.get("gr", 0.0),
                order=s["order"])


def _sum(terms):
    """terms: [(exact value, error its computed operand brings in, has a difference)] formed left to right -> (sum, e_sum)"""
    N = len(terms)
    total, e = 0.0, 0.0
    for j, (t, i, diff) in enumerate(terms):
        r = (1 if diff else 0) + 1 + (N - 1 if j < 2 else N - j)
        total = total + t
        e = e + i + 1.01 * r * U32 * (t.abs() + i)
    return total, e


def unipc_update(x, eu, et, last, hist, coef, gs, gr, order, depth=None):
    """x, eu, et (or None), last fp32 [batch, n]; hist fp32 [order, batch, n]; coef fp32 (12,); gs, gr as the C ABI passes them ->
    dict of float64 [batch, n]: out, e_out, xc, e_xc, mt, e_mt, E and the magnitudes accumulated() uses"""
    k = dict(zip(NAMES, coef.double().tolist()))
    E, e_E = guided(eu, et, gs, gr, depth)
    xd, zero = x.double(), torch.zeros_like(E)
    h = [hist[j].double() if j < order else None for j in range(3)]
    px = k["p"] * xd
    mt = px + k["q"] * E
    e_mt = abs(k["q"]) * e_E + 2 * U32 * (px.abs() + abs(k["q"]) * (E.abs() + e_E))
    mags = {}
    if k["corr"] != 0.0:
        terms = []
        if k["Ac"] != 0.0:
            terms.append((k["Ac"] * last.double(), zero, False))
        if k["Bc"] != 0.0:
            terms.append((k["Bc"] * h[0], zero, False))
        for name, j in (("C2", 1), ("C3", 2)):
            if k[name] != 0.0 and j < order:
                mags[name] = (h[j] - h[0]).abs()
                terms.append((k[name] * (h[j] - h[0]), zero, True))
        if k["Ct"] != 0.0:
            mags["Ct"] = (mt - h[0]).abs()
            terms.append((k["Ct"] * (mt - h[0]), abs(k["Ct"]) * e_mt, True))
        xc, e_xc = _sum(terms)
        xc, e_xc = xc + zero, e_xc + zero
    else:
        xc, e_xc = xd, zero
    terms = [(k["Ap"] * xc, abs(k["Ap"]) * e_xc, False), (k["Bp"] * mt, abs(k["Bp"]) * e_mt, False)]
    for name, j in (("D1", 0), ("D2", 1)):
        if k[name] != 0.0 and j < order:
            mags[name] = (h[j] - mt).abs()
            terms.append((k[name] * (h[j] - mt), abs(k[name]) * e_mt, True))
    out, e_out = _sum(terms)
    return dict(out=out, e_out=e_out, xc=xc, e_xc=e_xc, mt=mt, e_mt=e_mt, E=E, mags=mags)


def ratios(v, out, last, hist):
    """worst error / bound of one call's three results against the reference at the inputs v -> (out, last, plane 0, bits of the
    shifted planes that differ)"""
    from tests.rowmap_bounds import exact_off
    r = unipc_update(v["x"], v["eu"], v["et"], v["last"], v["hist"], v["coef"], v["gs"], v["gr"], v["order"])
    assert all(torch.isfinite(r[key]).all() for key in ("e_out", "e_xc", "e_mt"))
    shape = v["x"].shape
    hist = hist.reshape((v["order"],) + tuple(shape))
    off = sum(exact_off(hist[j], v["hist"][j - 1].to(hist.device)) for j in range(1, v["order"]))
    return (check(out.reshape(shape), r["out"], r["e_out"]), check(last.reshape(shape), r["xc"], r["e_xc"]),
            check(hist[0], r["mt"], r["e_mt"]), off)


def accumulated(xs, lasts, hists, outs, coef64, gs, gr, order, cfg=True):
    """The bound on |fused latents - float64 generic latents| after every step of a loop whose model outputs were replayed.
    xs[i], lasts[i], hists[i]: the fused loop's fp32 latents [B, ...], last [B, ...] and planes [order, B, ...] before step i
    (anything where the row does not use them); outs[i]: its fp32 model output ([2 B, ...] = [uncond, text] with cfg); coef64: the
    12 coefficients per step as Python floats -> list of float64 bounds shaped like the latents"""
    E_x = torch.zeros_like(xs[0], dtype=torch.float64).flatten(1)
    E_L, E_h = torch.zeros_like(E_x), [torch.zeros_like(E_x) for _ in range(3)]
    res = []
    for x, L, H, o, c64 in zip(xs, lasts, hists, outs, coef64):
        Bn = x.shape[0]
        c32 = torch.tensor(c64, dtype=torch.float32)
        xf, Lf, Hf = x.flatten(1), L.flatten(1), H.flatten(2)
        r = unipc_update(xf, o[:Bn].flatten(1), o[Bn:].flatten(1) if cfg else None, Lf, Hf, c32, gs, gr if cfg else 0.0, order)
        k = dict(zip(NAMES, c64))
        d = {n: abs(a - b) for n, a, b in zip(NAMES, c32.double().tolist(), c64)}
        m = r["mags"]
        dm = abs(k["p"]) * E_x + d["p"] * xf.double().abs() + d["q"] * r["E"].abs()
        if k["corr"] != 0.0:
            dxc = abs(k["Ac"]) * E_L + d["Ac"] * Lf.double().abs() + abs(k["Bc"]) * E_h[0] + d["Bc"] * Hf[0].double().abs()
            for name, j in (("C2", 1), ("C3", 2)):
                if name in m:
                    dxc = dxc + abs(k[name]) * (E_h[j] + E_h[0]) + d[name] * m[name]
            if "Ct" in m:
                dxc = dxc + abs(k["Ct"]) * (dm + E_h[0]) + d["Ct"] * m["Ct"]
            E_L_next = dxc + 2 * U32 * r["xc"].abs() + r["e_xc"]
        else:
            dxc = E_x
            E_L_next = E_x
        E_x = abs(k["Ap"]) * dxc + d["Ap"] * r["xc"].abs() + abs(k["Bp"]) * dm + d["Bp"] * r["mt"].abs() \
            + 2 * U32 * r["out"].abs() + r["e_out"]
        for name, j in (("D1", 0), ("D2", 1)):
            if name in m:
                E_x = E_x + abs(k[name]) * (E_h[j] + dm) + d[name] * m[name]
        E_L, E_h = E_L_next, [dm + 2 * U32 * r["mt"].abs() + r["e_mt"], E_h[0], E_h[1]]
        res.append(E_x.reshape(x.shape))
    return res
