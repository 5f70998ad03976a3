"""The elementwise fp64 bound of tests/attn_bounds.py, checked on the CPU against an emulation of the flash loop of csrc/attention.hip
(64-key tiles, the lazy reference with its RESCALE_THR / LAZY_PSUM_LIMIT logic, P rounded to the element type, l summed from the
unrounded fp32 exponentials, the online rescale, o * (1 / l), the accumulating form), on scaled-down versions of every case kind of
tests/attn_cases.py: the emulation stays inside the bound, and each injected indexing fault lands far outside it on the case kind
built to expose it."""
import math

import pytest
import torch

from tests import attn_bounds as AB
from tests import attn_cases as AC

KVBLK, QBLK = 64, 128
RESCALE_THR = 4.0
LIMIT = {torch.bfloat16: 2.0 ** 60, torch.float16: 2.0 ** 15}


def emulate(c, dt, lazy=True, fault=None):
    """the kernel's arithmetic on the inputs of attn_cases.make(); fault: tail | drop | rowshift | noalpha | bias_qstride |
    accum2 | old_row | colswap"""
    q, k, v, bias = c["q"], c["k"], c["v"], c["bias"]
    B, Sq, H, D = q.shape
    Skv = k.shape[1]
    sc = AB.fp32(c["scale"])
    c2 = 1.0 if c["log2"] else AB.fp32(sc * AC.LOG2E)
    inv = AB.fp32(1.0 / sc)
    ntiles = (Skv + KVBLK - 1) // KVBLK
    nfull = Skv // KVBLK
    out = torch.empty(B, Sq, H, D, dtype=dt)
    for b in range(B):
        for h in range(H):
            Q, K, V = q[b, :, h].float(), k[b, :, h].float(), v[b, :, h].float()
            n = ntiles * KVBLK
            Kp, Vp = torch.zeros(n, D), torch.zeros(n, D)
            Kp[:Skv], Vp[:Skv] = K, V
            S = (Q.double() @ Kp.double().t()).float()
            if bias is not None:
                bb = bias[b if bias.shape[0] > 1 else 0, h if bias.shape[1] > 1 else 0].expand(Sq, Skv).float()
                if fault == "bias_qstride":
                    bb = bb[:1].expand(Sq, Skv)
                S[:, :Skv] = S[:, :Skv] + bb * inv
            if fault != "tail":
                S[:, Skv:] = -math.inf
            m = torch.full((Sq,), -math.inf)
            l = torch.zeros(Sq)
            o = torch.zeros(Sq, D)
            for t in range(ntiles):
                if fault == "drop" and t == nfull - 1:
                    continue
                cols = slice(t * KVBLK, (t + 1) * KVBLK)
                s = S[:, cols]
                exact = torch.ones(Sq, dtype=torch.bool)
                if lazy and t > 0:
                    e = torch.exp2(s * c2 - m[:, None] * c2)
                    psum = e.sum(1)
                    exact = ~(psum <= LIMIT[dt])   # (too large / inf / NaN: the guard)
                if exact.any():
                    mloc = s.max(1).values
                    grow = exact & ((t == 0) | ((mloc - m) * c2 > RESCALE_THR) | (m == -math.inf))
                    m_new = torch.maximum(m, mloc)
                    m_use = torch.where(m_new == -math.inf, torch.zeros_like(m_new), m_new)
                    alpha = torch.exp2((m - m_use) * c2)
                    alpha = torch.where(grow, alpha, torch.ones_like(alpha))
                    if not (fault == "noalpha" and t > 0):
                        o = o * alpha[:, None]
                    l = l * alpha
                    m = torch.where(grow, m_use, m)
                    ee = torch.exp2(s * c2 - m[:, None] * c2)
                    e = ee if not lazy or t == 0 else torch.where(exact[:, None], ee, e)
                P = e.to(dt).float()
                l = l + e.sum(1)
                o = o + P @ Vp[cols]
            res = torch.where(l[:, None] > 0, o * (1.0 / l)[:, None], torch.zeros_like(o))
            if fault == "rowshift":   # query row i computed from row i - 1 in the last, partial query block
                r0 = (Sq // QBLK) * QBLK
                res[r0 + 1:] = res[r0:-1].clone()
            if fault == "colswap":    # two head-dim columns of the padded 32-wide block of DP = 96 swapped
                res[:, [64, 65]] = res[:, [65, 64]]
            if c["accum"] is not None:
                a = AB.fp32(c["accum"])
                old = c["old"][b, :, h].float()
                if fault == "old_row":
                    old = torch.roll(old, 1, 0)
                res = old + a * res + (a * res if fault == "accum2" else 0)
            out[b, :, h] = res.to(dt)
    return out


def ratio(c, out):
    r, rel = AB.bound_check(out, c["q"], c["k"], c["v"], scale=c["scale"], bias=c["bias"], log2=c["log2"], accum=c["accum"],
                            old=c["old"], exact_p=c["exact_p"])
    return r, rel


DTS = [torch.bfloat16, torch.float16]
# (config, bias layout, log2, accum)
CONFIGS = {"plain": (None, False, None), "log2": (None, True, None), "bias": ("bhqk", False, None), "accum": (None, False, 0.6),
           "bias+accum": ("b11k", False, 0.6), "t5": ("1hqk", False, None), "unet": ("unet", False, None)}
KINDS = ["S1", "S2", "S2g", "S2b", "S3", "S4"]


def _spec(kind, cfg, Skv=130, D=40):
    layout, log2, accum = CONFIGS[cfg]
    return dict(B=2, H=2, Sq=150, Skv=1 if kind == "S3" else Skv, D=D, kind=kind, bias=layout, log2=log2, accum=accum)


def _cases():
    for cfg, (layout, _, _) in CONFIGS.items():
        for kind in KINDS:
            if kind == "S2b" and layout not in ("bhqk", "b11k", "1hqk"):
                continue
            if kind in ("S2", "S2g") and layout in ("keep", "unet"):
                continue
            for lazy in ((False,) if layout is not None else (True, False)):
                yield cfg, kind, lazy


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "fp16"])
@pytest.mark.parametrize("cfg,kind,lazy", list(_cases()), ids=lambda x: str(x))
def test_bound_accepts_the_flash_loop(dt, cfg, kind, lazy):
    c = AC.make(_spec(kind, cfg), dt, seed=len(cfg) + ord(kind[-1]))
    out = emulate(c, dt, lazy=lazy)
    r, rel = ratio(c, out)
    print(f"{cfg:<11} {kind:<4} lazy={lazy!s:<5} {str(dt)[6:]:<9} err/bound {r:.3f}  rel {rel:.2e}")
    assert r < 1.0, (cfg, kind, r)
    if kind == "S4":
        assert rel < (5e-3 if dt == torch.bfloat16 else 6e-4), rel
    if kind == "S3":   # one key: out == v bit for bit (plus `old` for the accumulating form)
        want = c["v"][:, :1].expand_as(out) if c["accum"] is None else None
        if want is not None:
            assert torch.equal(out, want)


def test_bound_accepts_the_padded_head_dims():
    """D = 72 (DP = 96: the padded head-dim block) and D = 8, the emulation inside the bound on the selector and uniform kinds"""
    for D in (8, 72, 104):
        for kind in ("S1", "S2", "S4"):
            c = AC.make(_spec(kind, "plain", Skv=193, D=D), torch.bfloat16, seed=D)
            r, _ = ratio(c, emulate(c, torch.bfloat16, lazy=False))
            assert r < 1.0, (D, kind, r)


FAULTS = [  # fault, case kind, config, Skv, D, lazy
    ("tail", "S1", "plain", 65, 40, True),
    ("tail", "S1", "plain", 130, 40, True),
    ("tail", "S1", "plain", 193, 64, False),
    ("drop", "S1", "plain", 193, 40, True),
    ("drop", "S1", "log2", 256, 64, True),
    ("rowshift", "S2", "plain", 130, 40, True),
    ("rowshift", "S2", "log2", 130, 64, True),
    ("noalpha", "S2g", "plain", 256, 40, True),
    ("noalpha", "S2g", "log2", 256, 64, True),
    ("noalpha", "S2", "plain", 256, 72, False),
    ("bias_qstride", "S2b", "bias", 130, 40, False),
    ("bias_qstride", "S2b", "t5", 130, 40, False),
    ("accum2", "S1", "accum", 130, 40, True),
    ("accum2", "S2", "accum", 130, 40, True),
    ("old_row", "S1", "accum", 130, 40, True),
    ("old_row", "S2", "bias+accum", 130, 40, False),
    ("colswap", "S2", "plain", 130, 72, False),
]


@pytest.mark.parametrize("dt", DTS, ids=["bf16", "fp16"])
@pytest.mark.parametrize("fault,kind,cfg,Skv,D,lazy", FAULTS, ids=lambda x: str(x))
def test_bound_rejects_the_fault(dt, fault, kind, cfg, Skv, D, lazy):
    c = AC.make(_spec(kind, cfg, Skv=Skv, D=D), dt, seed=Skv + D)
    good, _ = ratio(c, emulate(c, dt, lazy=lazy))
    bad, rel = ratio(c, emulate(c, dt, lazy=lazy, fault=fault))
    print(f"{fault:<13} {kind:<4} {cfg:<10} Skv {Skv:<4} D {D:<3} {str(dt)[6:]:<9} err/bound {good:.3f} -> {bad:.1f}  (rel {rel:.2e})")
    assert good < 1.0, good
    assert bad > 4.0, (fault, bad)


def test_selectors_select():
    """S2 / S2g: every query row's selected key leads the row by the stated margin (float64, on the rounded q)"""
    for kind, mg in (("S2", AC.MARGIN), ("S2g", AC.MARGIN_GUARD)):
        c = AC.make(dict(B=1, H=2, Sq=200, Skv=193, D=40, kind=kind), torch.bfloat16, seed=3)
        x = torch.einsum("bqhd,bkhd->bhqk", c["q"].double(), c["k"].double()) * AB.fp32(c["scale"])
        top = x.topk(2, -1).values
        assert ((top[..., 0] - top[..., 1]) >= mg).all()
        hit = set(x.argmax(-1).flatten().tolist())
        assert set(AC.tail_keys(193)) - ({0, 63} if kind == "S2g" else set()) <= hit, (kind, sorted(hit))


def test_whole_row_inf_mask_is_zero():
    """a row whose keys are all masked with -inf: the kernels write 0 (include/mi355x_sd.h), the reference says 0 with e = 0"""
    c = AC.make(_spec("S4", "bias"), torch.bfloat16, seed=9)
    c["bias"][0, 1, 7] = -math.inf
    out = emulate(c, torch.bfloat16, lazy=False)
    assert (out[0, 7, 1] == 0).all()
    r, _ = ratio(c, out)
    assert r < 1.0
