"""Child of tests/test_gpu_norms.py: the case matrix of the normalisation kernels (csrc/norm.hip, csrc/fused_ops.hip), each case held
to the elementwise float64 bound of tests/norm_bounds.py over its WHOLE output (the reference runs on the device). Outputs are views
inside buffers of the 0x7FA5 canary (row padding ldy > C, rows past the end); the input row gaps (ldx > C) and the modulation
vectors' gaps (ld_mod > C) hold NaN, so a read outside a row poisons the statistics. With MI355X_SD_NORM_LOG set (debug build) each
case also reports the kernel instantiations its launcher logged. Prints one JSON line: per case worst err / bound (and of the
side outputs), unwritten / overwritten element counts, bit checks, route, and "sha": a digest (tests/gpu_child.sha) of every output
tensor the case checks -- what a comparison of two builds' bits reads.

  python tests/norm_child.py [case ...]     (no names: every case)
"""
import functools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from paddlemix_amd import _lib, ops  # noqa: E402
from tests import norm_bounds as NB  # noqa: E402
from tests import kernel_pieces as KP  # noqa: E402
from tests.gpu_child import sha  # noqa: E402

EPS = 1e-5
CASES = {}        # name: (entry, spec, the route lines the log must show, without C)


def _add(name, entry, route, **spec):
    CASES[name] = (entry, spec, route)


def _nch(entry, C):
    return NB.nch(entry, C)


# ---- GroupNorm, split form: gn_partial_kernel<XF32> + gn_finalize_kernel + scale_shift_act_kernel<SILU, XF32> ------------------
def _gn(name, B, HW, C, groups, xf32, silu, kind="random", r=0.0, raw16=False):
    act = ("silu," if silu else "id,") + ("xf32" if xf32 else "x16")
    route = [f"gn_partial 0 0 {'xf32' if xf32 else 'x16'}", "gn_finalize 0 0 -", f"scale_shift_act 0 0 {act}"]
    _add(name, "gn", route, B=B, HW=HW, C=C, groups=groups, xf32=xf32, silu=silu, kind=kind, r=r, raw16=raw16)


_gn("gn C320 idle threads x16 silu", 2, 1024, 320, 32, False, True)
_gn("gn C320 HW1000 ragged xf32 r1000 raw16", 1, 1000, 320, 32, True, True, r=1000.0, raw16=True)
_gn("gn C320 HW3 below ppp x16 r16", 2, 3, 320, 32, False, False, r=16.0)
_gn("gn C2056 ppp1 xf32 r4096", 1, 50, 2056, 8, True, False, r=4096.0)
_gn("gn C4096 maxc 64 groups x16 r256", 1, 40, 4096, 64, False, True, r=256.0)
_gn("gn groups1 x16 pilot outlier", 2, 300, 64, 1, False, False, kind="outlier0")
_gn("gn groups64 xf32 r1000 raw16", 1, 200, 1280, 64, True, False, r=1000.0, raw16=True)
_gn("gn x16 outlier elsewhere r256", 1, 256, 640, 32, False, True, kind="outlier", r=256.0)
_gn("gn xf32 outlier elsewhere r4096", 1, 256, 640, 32, True, True, kind="outlier", r=4096.0)
_gn("gn x16 constant", 1, 64, 640, 32, False, False, kind="const", r=3.0)
_gn("gn xf32 plus-minus", 1, 64, 640, 32, True, False, kind="pm", r=2.0)
_gn("gn x16 near-constant", 1, 64, 640, 32, False, False, kind="nearconst", r=1.0)
_gn("gn x16 large silu", 2, 256, 320, 32, False, True, kind="silu_big")
_gn("gn xf32 large silu raw16", 1, 256, 320, 32, True, True, kind="silu_big", raw16=True)
_gn("gn cpg 4 straddling chunks xf32", 1, 100, 128, 32, True, False, kind="outlier0", r=1000.0)


# ---- GroupNorm, one launch: gn_fused_kernel<SILU> ----------------------------------------------------------------------------
def _gnf(name, B, HW, C, groups, silu, kind="random", r=0.0, refused=False):
    route = [] if refused else [f"gn_fused 0 0 {'silu' if silu else 'id'}"] * ((B + 65534) // 65535)
    _add(name, "gnf", route, B=B, HW=HW, C=C, groups=groups, silu=silu, kind=kind, r=r, refused=refused)


_gnf("gnf cpg2 dpp1 silu", 2, 300, 64, 32, True)
_gnf("gnf cpg2 dpp1 pilot outlier r256", 1, 200, 64, 32, False, kind="outlier0", r=256.0)
_gnf("gnf cpg128 at 24576 r16", 2, 384, 256, 2, False, r=16.0)
_gnf("gnf cpg128 at 24576 silu outlier", 1, 384, 256, 2, True, kind="outlier", r=16.0)
_gnf("gnf cpg128 one over is refused", 1, 385, 256, 2, False, refused=True)
_gnf("gnf B65538 HW1 grid slices", 65538, 1, 8, 4, True)
_gnf("gnf constant", 1, 100, 640, 32, False, kind="const", r=3.0)
_gnf("gnf near-constant silu", 1, 100, 640, 32, True, kind="nearconst", r=1.0)
_gnf("gnf large silu", 2, 256, 320, 32, True, kind="silu_big")


# ---- row kernels --------------------------------------------------------------------------------------------------------------
def _ln(name, rows, C, xf32, affine=True, kind="random", r=0.0):
    _add(name, "ln", [f"layernorm {_nch('layernorm', C)} 2 {'xf32' if xf32 else 'x16'}"], rows=rows, C=C, xf32=xf32, affine=affine,
         kind=kind, r=r)


for i, C in enumerate((1024, 1032, 1536, 1544, 2560)):
    for xf32 in (False, True):
        kinds = (("random", 0.0), ("outlier0", 16.0), ("outlier", 256.0), ("pm", 1.0), ("nearconst", 1.0)) if not xf32 else \
            (("random", 1000.0), ("outlier0", 4096.0), ("outlier", 1000.0), ("pm", 4096.0), ("random", 0.0))
        kind, r = kinds[i]
        _ln(f"ln C{C} {'xf32' if xf32 else 'x16'} {kind} r{r:g}", (1, 3, 5, 77, 300)[i], C, xf32, affine=(i % 2 == 0), kind=kind, r=r)
_ln("ln looping waves x16", 8200, 1024, False, r=16.0)
_ln("ln looping waves xf32", 8195, 1032, True, r=1000.0)
_ln("ln constant rows", 5, 1024, False, kind="const", r=2.0)
_ln("ln constant rows xf32 no affine", 3, 1544, True, affine=False, kind="const", r=1000.0)


def _rs(name, rows, C, kind="random", r=0.0):
    _add(name, "rs", [f"row_stats {_nch('row_stats', C)} 4 -"], rows=rows, C=C, kind=kind, r=r)


for i, C in enumerate((512, 520, 1024, 1032, 1536, 1544, 2560)):
    kind, r = (("random", 0.0), ("outlier0", 16.0), ("outlier", 256.0), ("pm", 1.0), ("nearconst", 1.0), ("random", 256.0),
               ("outlier0", 256.0))[i]
    _rs(f"rs C{C} {kind} r{r:g}", (1, 3, 5, 77, 300, 2, 4)[i], C, kind, r)
_rs("rs looping waves", 16390, 512, r=16.0)


def _rms(name, rows, C, kind="random"):
    _add(name, "rms", [f"rmsnorm {_nch('rmsnorm', C)} 2 -"], rows=rows, C=C, kind=kind, r=0.0)


for i, C in enumerate((1024, 1032, 2048, 2056, 4096)):
    _rms(f"rms C{C} {('random', 'big', 'zero_row', 'random', 'big')[i]}", (1, 3, 5, 77, 300)[i], C,
         ("random", "big", "zero_row", "random", "big")[i])
_rms("rms looping waves", 8200, 1024, "zero_row")


def _ad(name, rows, C, m16, rpb, kind="random", r=0.0):
    R = 2 if C // 8 > 192 else 4
    _add(name, "ad", [f"adaln {_nch('adaln', C)} {R} {'m16' if m16 else 'm32'}"], rows=rows, C=C, m16=m16, rpb=rpb, kind=kind, r=r)


for C in (1024, 1536, 2560):
    for m16 in (False, True):
        t = "m16" if m16 else "m32"
        _ad(f"ad C{C} {t} rpb77", 2 * 77 + 3, C, m16, 77, "outlier0" if m16 else "random", 16.0)
        _ad(f"ad C{C} {t} rpb154", 3 * 154, C, m16, 154, "outlier" if m16 else "pm", 256.0 if m16 else 1.0)
_ad("ad rows 1", 1, 1024, False, 77)
_ad("ad rows 3 rpb 2", 3, 1536, True, 2, "nearconst", 1.0)
_ad("ad rows 5", 5, 2560, False, 4)
_ad("ad looping waves rpb4250", 33000, 1024, True, 4250, r=16.0)
_ad("ad looping waves C2560", 16400, 2560, False, 4250)
_ad("ad constant rows", 200, 1024, False, 77, "const", 3.0)


def _af8(name, rows, C, l2, kind="random", r=0.0):
    _add(name, "af8", [f"adaln_f8 {_nch('adaln_f8', C)} 1 -"], rows=rows, C=C, l2=l2, kind=kind, r=r, rpb=77)


_af8("af8 C1024 yl2", 157, 1024, True)
_af8("af8 C1024 no yl2 outlier", 80, 1024, False, "outlier", 16.0)
_af8("af8 C1536 yl2 pilot outlier", 157, 1536, True, "outlier0", 256.0)
_af8("af8 C1536 no yl2", 3, 1536, False)
_af8("af8 C2560 yl2 plus-minus", 5, 2560, True, "pm", 1.0)
_af8("af8 C2560 no yl2", 1, 2560, False)
_af8("af8 looping waves", 8200, 1024, True, r=16.0)


def _q8(name, rows, C, rpb, kind="random"):
    _add(name, "q8", ["quantize_rows 0 1 -"], rows=rows, C=C, rpb=rpb, kind=kind, r=0.0)


_q8("q8 compact exact max", 300, 1024, 0, "q_exactmax")
_q8("q8 remapped zero rows", 2 * 77 + 5, 1536, 77, "q_zero")
_q8("q8 subnormal e4m3", 77, 520, 0, "q_tiny")
_q8("q8 looping waves remapped", 8200, 64, 4100, "q_tiny")


def _fa(name, rows, C, m16, affine, kind="random", r=0.0):
    _add(name, "fa", [f"fused_adaln {_nch('fused_adaln', C)} 1 {'m16' if m16 else 'm32'}"], rows=rows, C=C, m16=m16, affine=affine,
         kind=kind, r=r, rpb=77)


for i, C in enumerate((1024, 1032, 2048, 2056, 4096)):
    for m16 in (False, True):
        kind, r = (("random", 0.0), ("outlier0", 16.0), ("outlier", 256.0), ("pm", 1.0), ("random", 16.0))[i]
        _fa(f"fa C{C} {'m16' if m16 else 'm32'} {kind}", (1, 3, 5, 157, 300)[i] + m16, C, m16, affine=(i + m16) % 2 == 0,
            kind=kind, r=r)
_fa("fa looping waves", 8200, 1024, True, True, r=16.0)
_fa("fa constant rows", 5, 1024, False, False, "const", 3.0)


# ---- buffers ------------------------------------------------------------------------------------------------------------------
def _canary(shape, ld, kind):
    """a [rows, C] or [B, HW, C] view with row stride ld in a flat canary buffer, 3 extra rows and 64 elements behind: (view, guard)"""
    g = KP.Guarded.rows(shape, ld, kind, extra_rows=3, tail=64, dt=_lib.elem_dtype())
    return g.view, g


_nan_rows = functools.partial(KP.nan_rows, tail=64)   # (vals [..., C], ld) -> a view with row stride ld in a NaN buffer, 64 NaN behind


def _values(shape, kind, r, dt, g):
    """the input values (exact in dt) of each input kind"""
    C = shape[-1]
    x = torch.randn(shape, generator=g, device="cuda")
    if kind == "random":
        x = x + r
    elif kind == "outlier0":       # the pilot (row start / pixel 0, channel 0) is a 50 sigma outlier
        x = x + r
        if x.dim() == 3:
            x[:, 0, 0] = r + 50.0
        else:
            x[:, 0] = r + 50.0
    elif kind == "outlier":        # a 50 sigma outlier elsewhere
        x = x + r
        if x.dim() == 3:
            x[:, x.shape[1] // 2, C // 2 + 3] = r + 50.0
        else:
            x[:, C // 2 + 3] = r + 50.0
    elif kind == "const":
        x = torch.full(shape, r + 0.75, device="cuda")
    elif kind == "pm":             # +-a around r: exact variance a^2
        x = r + torch.where(torch.arange(C, device="cuda") % 2 == 0, 1.5, -1.5).expand(shape).clone()
    elif kind == "nearconst":      # var = 2^-16 << eps... ~ eps
        x = r + 2.0 ** -7 * (torch.rand(shape, generator=g, device="cuda") < 0.5).float()
    elif kind == "silu_big":
        x = 3 * x
    elif kind == "big":
        x = 1e4 * (1 + 0.1 * x) * torch.where(torch.rand(shape, generator=g, device="cuda") < 0.5, 1.0, -1.0)
    elif kind == "zero_row":
        x[1::2] = 0.0
    elif kind == "q_exactmax":
        x = x.clamp(-3.0, 3.0)
        x[:, 7] = -3.5                                         # the row maximum: exactly representable, a power of 2 apart
        x = x * 2.0 ** (torch.arange(shape[0], device="cuda") % 9 - 4).float()[:, None]
    elif kind == "q_zero":
        x[::3] = 0.0
    elif kind == "q_tiny":         # tiny values beside a large maximum: the subnormal e4m3 range
        x = x * 2.0 ** -12
        x[:, 1] = 100.0
    return x.to(dt)


def _gamma_beta(C, g, big=False):
    gamma = (1 + 0.3 * torch.randn(C, generator=g, device="cuda")) * (30.0 if big else 1.0)
    beta = 0.3 * torch.randn(C, generator=g, device="cuda")
    return gamma.float(), beta.float()


def _mod(nb, C, m16, g, scale=0.5, ld_pad=24):
    """[nb, C] modulation vectors (fp32 or 16-bit) as a strided view of rows ld_mod = C + ld_pad with NaN gaps"""
    ed = _lib.elem_dtype()
    v = (scale * torch.randn(nb, C, generator=g, device="cuda")).to(ed if m16 else torch.float32)
    return _nan_rows(v, C + ld_pad)


# ---- cases --------------------------------------------------------------------------------------------------------------------
def run_case(name):
    entry, s, _ = CASES[name]
    lib = _lib.load()
    ed = _lib.elem_dtype()
    st = ops._stream()
    g = torch.Generator(device="cuda").manual_seed(sum(map(ord, name)))
    res = {}
    if entry in ("gn", "gnf"):
        B, HW, C, groups = s["B"], s["HW"], s["C"], s["groups"]
        xdt = torch.float32 if s.get("xf32") else ed
        vals = _values((B, HW, C), s["kind"], s["r"], xdt, g)
        gamma, beta = _gamma_beta(C, g, s["kind"] == "silu_big")
        ldx = C + (8 if entry == "gn" else 2)
        x = _nan_rows(vals, ldx)
        y, ybits = _canary((B, HW, C), C + 8, 16)
        if entry == "gn":
            ws = torch.empty(max(1, lib.mi355x_sd_groupnorm_workspace_floats(B, HW, C)), device="cuda")
            ss = torch.empty((B, 2, C), device="cuda")
            rc = lib.mi355x_sd_groupnorm_stats_ex(x.data_ptr(), B, HW, C, ldx, groups, EPS, gamma.data_ptr(), beta.data_ptr(),
                                                  ws.data_ptr(), ss.data_ptr(), 1 if s["xf32"] else 0, st)
            raw = rbits = None
            if s["raw16"]:
                raw, rbits = _canary((B, HW, C), C + 16, 16)
            rc = rc or lib.mi355x_sd_scale_shift_act_ex(x.data_ptr(), B, HW, C, ldx, ss.data_ptr(), 1 if s["silu"] else 0,
                                                        y.data_ptr(), C + 8, 1 if s["xf32"] else 0,
                                                        raw.data_ptr() if raw is not None else None, C + 16, st)
            L = NB.chain_gn_split(HW, C, groups)
        else:
            rc = lib.mi355x_sd_groupnorm_act(x.data_ptr(), B, HW, C, ldx, groups, EPS, gamma.data_ptr(), beta.data_ptr(),
                                             1 if s["silu"] else 0, y.data_ptr(), C + 8, st)
            L = NB.chain_gn_fused()
        torch.cuda.synchronize()
        res["rc"] = rc
        if s.get("refused"):   # nothing written anywhere
            res["unwritten"], res["overwritten"] = 0, int((ybits.bits != ybits.canary).sum().item())
            return res
        ref, e = NB.groupnorm(vals, gamma, beta, groups, EPS, s["silu"], L=L)
        res["ratio"], res["rel"] = NB.check(y, ref, e)
        res["unwritten"], res["overwritten"] = ybits.counts()
        res["sha"] = {"y": sha(y)}
        if entry == "gn" and s["raw16"]:
            res["sha"]["raw16"] = sha(raw)
            uw, ow = rbits.counts()
            res["unwritten"] += uw
            res["overwritten"] += ow
            res["raw16_exact"] = bool(torch.equal(raw.contiguous().view(torch.int16), vals.to(ed).view(torch.int16)))
        return res

    rows, C = s["rows"], s["C"]
    if entry == "ln":
        xdt = torch.float32 if s["xf32"] else ed
        vals = _values((rows, C), s["kind"], s["r"], xdt, g)
        gamma, beta = _gamma_beta(C, g) if s["affine"] else (None, None)
        x = _nan_rows(vals, C + 16)
        y, bits = _canary((rows, C), C + 8, 16)
        res["rc"] = lib.mi355x_sd_layernorm_ex(x.data_ptr(), rows, C, C + 16, ops._p(gamma), ops._p(beta), EPS, y.data_ptr(), C + 8,
                                               1 if s["xf32"] else 0, st)
        torch.cuda.synchronize()
        res["sha"] = {"y": sha(y)}
        ref, e = NB.layernorm(vals, gamma, beta, EPS, NB.chain_rows("layernorm", C))
        res["ratio"], res["rel"] = NB.check(y, ref, e)
        res["unwritten"], res["overwritten"] = bits.counts()
        if s["kind"] == "const":   # z' = 0 exactly: y = beta
            want = (beta if beta is not None else torch.zeros(C, device="cuda")).to(ed).expand(rows, C)
            res["exact"] = bool(torch.equal(y.contiguous().view(torch.int16), want.contiguous().view(torch.int16)))
    elif entry == "rs":
        vals = _values((rows, C), s["kind"], s["r"], ed, g)
        x = _nan_rows(vals, C + 8)
        y, bits = _canary((rows, 2), 2, 32)
        res["rc"] = lib.mi355x_sd_row_stats(x.data_ptr(), rows, C, C + 8, EPS, y.data_ptr(), st)
        torch.cuda.synchronize()
        res["sha"] = {"stats": sha(y)}
        ref, e = NB.row_stats(vals, EPS, NB.chain_rows("row_stats", C))
        res["ratio"], res["rel"] = NB.check(y, ref, e, u_out=0.0)
        res["unwritten"], res["overwritten"] = bits.counts()
    elif entry == "rms":
        vals = _values((rows, C), s["kind"], s["r"], ed, g)
        w = (1 + 0.3 * torch.randn(C, generator=g, device="cuda")).float()
        x = _nan_rows(vals, C + 24)
        y, bits = _canary((rows, C), C + 8, 16)
        res["rc"] = lib.mi355x_sd_rmsnorm(x.data_ptr(), rows, C, C + 24, w.data_ptr(), 1e-6, y.data_ptr(), C + 8, st)
        torch.cuda.synchronize()
        res["sha"] = {"y": sha(y)}
        ref, e = NB.rmsnorm(vals, w, 1e-6, NB.chain_rows("rmsnorm", C))
        res["ratio"], res["rel"] = NB.check(y, ref, e)
        res["unwritten"], res["overwritten"] = bits.counts()
        if s["kind"] == "zero_row":
            res["exact"] = bool((y[1::2].float() == 0).all().item())
    elif entry == "ad":
        rpb = s["rpb"]
        nb = (rows + rpb - 1) // rpb
        vals = _values((rows, C), s["kind"], s["r"], ed, g)
        x = _nan_rows(vals, C + 8)
        sc, sh = _mod(nb, C, s["m16"], g), _mod(nb, C, s["m16"], g, scale=2.0)
        y, bits = _canary((rows, C), C + 8, 16)
        res["rc"] = lib.mi355x_sd_adaln_ex(x.data_ptr(), rows, C, C + 8, sc.data_ptr(), sh.data_ptr(), sc.stride(0),
                                           _lib.MOD_ELEM if s["m16"] else _lib.MOD_F32, rpb, 1e-6, y.data_ptr(), C + 8, st)
        torch.cuda.synchronize()
        res["sha"] = {"y": sha(y)}
        ref, e = NB.adaln(vals, sc, sh, rpb, 1e-6, NB.chain_rows("adaln", C))
        res["ratio"], res["rel"] = NB.check(y, ref, e)
        res["unwritten"], res["overwritten"] = bits.counts()
        if s["kind"] == "const":   # y = shift[b]
            want = sh.to(ed)[torch.arange(rows, device="cuda") // rpb]
            res["exact"] = bool(torch.equal(y.contiguous().view(torch.int16), want.contiguous().view(torch.int16)))
    elif entry == "af8":
        rpb = s["rpb"]
        nb = (rows + rpb - 1) // rpb
        vals = _values((rows, C), s["kind"], s["r"], ed, g)
        x = _nan_rows(vals, C + 8)
        sc, sh = _mod(nb, C, False, g), _mod(nb, C, False, g, scale=2.0)
        y8, bits = _canary((rows, C), C + 16, 8)
        qs, qbits = _canary((rows, 1), 1, 32)
        l2 = l2bits = None
        if s["l2"]:
            l2, l2bits = _canary((rows, 1), 1, 32)
        res["rc"] = lib.mi355x_sd_adaln_f8(x.data_ptr(), rows, C, C + 8, sc.data_ptr(), sh.data_ptr(), sc.stride(0), rpb, 1e-6,
                                           y8.data_ptr(), C + 16, qs.data_ptr(), l2.data_ptr() if l2 is not None else None, st)
        torch.cuda.synchronize()
        res["sha"] = {"y8": sha(y8), "yscale": sha(qs)}
        if l2 is not None:
            res["sha"]["yl2"] = sha(l2)
        ref, e = NB.adaln_pre(vals, sc, sh, rpb, 1e-6, NB.chain_rows("adaln_f8", C))
        r_val, r_qs, r_l2, nan = NB.check_f8(y8, qs[:, 0], l2[:, 0] if l2 is not None else None, ref, e)
        res["ratio"], res["ratio_qs"], res["ratio_l2"], res["nan_bytes"] = r_val, r_qs, r_l2, nan
        res["unwritten"] = qbits.counts()[0] + (l2bits.counts()[0] if l2 is not None else 0)
        res["overwritten"] = (bits.counts()[1] + qbits.counts()[1]
                              + (l2bits.counts()[1] if l2 is not None else 0))
    elif entry == "q8":
        rpb = s["rpb"]
        vals = _values((rows, C), s["kind"], s["r"], ed, g)
        if rpb:   # source rows of one stream inside a [B, rpb + 11, C + 8] tensor: row m at (m / rpb) * bstride + (m % rpb) * ldx
            nb = (rows + rpb - 1) // rpb
            src = torch.full((nb, rpb + 11, C + 8), float("nan"), device="cuda").to(ed)
            flat = src[:, :rpb, :C].reshape(nb * rpb, C)
            flat[:rows] = vals
            src[:, :rpb, :C] = flat.reshape(nb, rpb, C)
            xp, ldx, bst = src.data_ptr(), C + 8, (rpb + 11) * (C + 8)
        else:
            x = _nan_rows(vals, C + 8)
            xp, ldx, bst = x.data_ptr(), C + 8, 0
        y8, bits = _canary((rows, C), C + 8, 8)
        qs, qbits = _canary((rows, 1), 1, 32)
        res["rc"] = lib.mi355x_sd_quantize_rows(xp, rows, C, ldx, rpb, bst, y8.data_ptr(), C + 8, qs.data_ptr(), st)
        torch.cuda.synchronize()
        res["sha"] = {"y8": sha(y8), "yscale": sha(qs)}
        q_ref, qs_ref = NB.quantize_rows_exact(vals)
        got = y8.contiguous().cpu()
        res["exact_bytes_off"] = int((got != q_ref).sum().item())
        res["exact_scale_off"] = int((qs[:, 0].cpu() != qs_ref).sum().item())
        res["nan_bytes"] = int(((got & 0x7F) == 0x7F).sum().item())
        res["ratio"], _, _, _ = NB.check_f8(y8, qs[:, 0], None, vals.double(), torch.zeros_like(vals, dtype=torch.float64))
        res["unwritten"] = qbits.counts()[0]
        res["overwritten"] = bits.counts()[1] + qbits.counts()[1]
    elif entry == "fa":
        rpb = s["rpb"]
        nb = (rows + rpb - 1) // rpb
        xv = _values((rows, C), s["kind"], s["r"], ed, g)
        mv = (torch.randn(rows, C, generator=g, device="cuda") * (0 if s["kind"] == "const" else 1)).to(ed)
        x, mha = _nan_rows(xv, C + 8), _nan_rows(mv, C + 16)
        gate, sc, sh = _mod(nb, C, s["m16"], g, scale=0.3), _mod(nb, C, s["m16"], g), _mod(nb, C, s["m16"], g, scale=2.0)
        w = b = None
        if s["affine"]:
            mdt = ed if s["m16"] else torch.float32
            w, b = (1 + 0.3 * torch.randn(C, generator=g, device="cuda")).to(mdt), (0.3 * torch.randn(C, generator=g, device="cuda")).to(mdt)
        resi, rbits = _canary((rows, C), C + 8, 16)
        y, bits = _canary((rows, C), C + 24, 16)
        res["rc"] = lib.mi355x_sd_fused_adaln_scale_residual_ex(
            x.data_ptr(), C + 8, mha.data_ptr(), C + 16, gate.data_ptr(), sc.data_ptr(), sh.data_ptr(), gate.stride(0),
            _lib.MOD_ELEM if s["m16"] else _lib.MOD_F32, rpb, ops._p(w), ops._p(b), EPS, rows, C, resi.data_ptr(), C + 8,
            y.data_ptr(), C + 24, st)
        torch.cuda.synchronize()
        res["sha"] = {"resi": sha(resi), "out": sha(y)}
        rref, re_ = NB.fused_resi(xv, mv, gate, rpb)
        res["ratio_resi"], _ = NB.check(resi, rref, re_)
        ref, e = NB.fused_adaln_out(resi.float(), sc, sh, rpb, w, b, EPS, NB.chain_rows("fused_adaln", C))
        res["ratio"], res["rel"] = NB.check(y, ref, e)
        uw, ow = bits.counts()
        uw2, ow2 = rbits.counts()
        res["unwritten"], res["overwritten"] = uw + uw2, ow + ow2
        if s["kind"] == "const":   # mha = 0: resi = x, z' = 0, y = shift[b]
            want = sh.to(ed)[torch.arange(rows, device="cuda") // rpb]
            res["exact"] = bool(torch.equal(y.contiguous().view(torch.int16), want.contiguous().view(torch.int16)))
    return res


if __name__ == "__main__":
    KP.run_cases(CASES, run_case, route_log="MI355X_SD_NORM_LOG", tag="NORM_JSON", names=sys.argv[1:])
