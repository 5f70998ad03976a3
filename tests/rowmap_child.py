"""Child of tests/test_gpu_rowmaps.py: the case matrix of the row-map and layout kernels (csrc/misc.hip outside the direct
convolutions, split_concat of csrc/fused_ops.hip). Bound-class cases are held to the elementwise float64 bounds of
tests/rowmap_bounds.py over their WHOLE output, exact-class cases to its torch restatements bit for bit (references run on the
device). Outputs are views inside buffers of the 0x7FA5 / 0x7FA5A5A5 canary (row padding ld > C, everything after the last row);
input row gaps and the space after every floating-point input hold NaN. Every grid-stride kernel runs below one block, ragged just
over one block, and ragged over its launcher's block cap x 256 work items (a second trip of the loop). Prints one JSON line: per
case the worst err / bound or the number of differing elements, and the unwritten / overwritten element counts.

  python tests/rowmap_child.py [case ...]     (no names: every case)
"""
import functools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from paddlemix_amd import _lib, ops  # noqa: E402
from tests import rowmap_bounds as RB  # noqa: E402
from tests import kernel_pieces as KP  # noqa: E402

CASES = {}   # name: (family, spec)
F32 = torch.float32


def _add(name, family, **spec):
    assert name not in CASES, name
    CASES[name] = (family, spec)


def _over(kernel, extra):
    """work items: the launcher's block cap x 256 plus a ragged `extra`"""
    return RB.GRID_CAP[kernel] * RB.BLOCK + extra


# ---- the matrix -----------------------------------------------------------------------------------------------------------------
for fi, fo in ((0, 0), (0, 1), (1, 0), (1, 1)):
    tag = f"{'f32' if fi else 'x16'}->{'f32' if fo else 'x16'}"
    _add(f"silu {tag} all values", "silu", n="sweep", in_f32=fi, out_f32=fo)
    for n in (200, 293, _over("silu", 777)):
        _add(f"silu {tag} n{n}", "silu", n=n, in_f32=fi, out_f32=fo)
for kind in ("quick_gelu", "gelu", "silu"):
    _add(f"act {kind} all values", "act", kind=kind, n="sweep")
for kind, n8 in (("quick_gelu", 30), ("gelu", 300), ("silu", _over("activation", 77))):
    _add(f"act {kind} n8 {n8}", "act", kind=kind, n=8 * n8)
for kind in ("quick_gelu", "gelu", "silu", "gelu_new"):
    _add(f"gated {kind} all values ldx>2F", "gated", kind=kind, rows="sweep", F=64, xpad=16)
_add("gated gelu_new all values ldx=2F", "gated", kind="gelu_new", rows="sweep", F=64, xpad=0)
for kind, rows, F in (("gelu", 3, 8), ("silu", 5, 520), ("gelu_new", 4099, 2056)):   # 3, 325, 4096 * 256 + 4867 work items
    _add(f"gated {kind} rows{rows} F{F}", "gated", kind=kind, rows=rows, F=F, xpad=24)
for n in (4, 1020, 1028, 16384):
    _add(f"softmax n{n}", "softmax", n=n)
TS = (0.0, 1.0, 999.0, 500.5, 0.25, 37.75)
for name, spec in (
        ("dim2 shift0 flip", dict(dim=2, shift=0.0, flip=1)),
        ("dim64 shift1", dict(dim=64, shift=1.0, flip=0)),
        ("dim320 shift0 flip", dict(dim=320, shift=0.0, flip=1)),
        ("dim320 shift1 period100", dict(dim=320, shift=1.0, flip=0, period=100.0)),
        ("dim321 odd shift1 flip", dict(dim=321, shift=1.0, flip=1)),
        ("dim321 odd shift0 period1000", dict(dim=321, shift=0.0, flip=0, period=1000.0)),
        ("dim256 group6 ldo wide", dict(dim=256, shift=0.0, flip=1, group=6, n=12, t=(1024.0, 1024.0, 0.0, 0.0, 768.0, 1344.5) * 2)),
        ("dim64 group6 t_count<n", dict(dim=64, shift=1.0, flip=1, group=6, n=18)),
        ("dim320 t_count1 n5", dict(dim=320, shift=0.0, flip=1, n=5, t=(801.0,))),
        ("dim256 scale1000", dict(dim=256, shift=1.0, flip=1, scale=1000.0, t=(0.0, 0.001, 0.5, 0.999, 1.0, 0.12345)))):
    _add("temb " + name, "temb", **spec)
for n in (100, 300, _over("axpby", 333)):
    _add(f"axpby n{n}", "axpby", n=n, coef=(0.25, -1.5), kind="random", alias=False)
    _add(f"axpby n{n} cancelling in place", "axpby", n=n, coef=(1.5, -1.5), kind="cancel", alias=True)
    for gs in (0.0, 1.0, 7.5):
        _add(f"cfg n{n} gs{gs:g}", "cfg", n=n, coef=(1.0127, -0.0423) if gs else (1.5, -1.5), gs=gs)
for B, L, HW in ((2, 4, 5), (1, 4, 67), (2, 4, _over("latent_dist", 448) // 8)):
    for noise in (True, False):
        _add(f"latent B{B} L{L} HW{HW} {'noise' if noise else 'mode'}", "latent", B=B, L=L, HW=HW, noise=noise)
for rows, C in ((3, 8), (5, 520), (4099, 2056)):
    _add(f"copy_rows {rows}x{C}", "copy", rows=rows, C=C)
    _add(f"cast_rows {rows}x{C}", "cast", rows=rows, C=C)
for B, C, H, W, p, pad in ((2, 3, 5, 7, 1, 8), (2, 3, 5, 9, 1, 0), (2, 16, 6, 10, 2, 8), (2, 3, 8, 12, 4, 8), (2, 16, 8, 12, 4, 16),
                           (2, 3, 598, 586, 2, 8)):
    _add(f"patchify B{B} C{C} {H}x{W} p{p} pad{pad}", "patchify", B=B, C=C, H=H, W=W, p=p, pad=pad)
    _add(f"unpatchify B{B} C{C} {H}x{W} p{p} pad{pad}", "unpatchify", B=B, C=C, H=H, W=W, p=p, pad=pad)
for B, S1, S2, C in ((2, 3, 0, 8), (2, 0, 5, 8), (3, 7, 9, 16), (3, 20000, 9130, 64)):
    _add(f"split_concat B{B} S{S1}+{S2} C{C}", "split", B=B, S1=S1, S2=S2, C=C)
for n, seq, V, D in ((10, 7, 50, 8), (45, 20, 300, 64), (131200, 77, 400, 64)):
    for mode in ("tok", "tok+pos", "pos"):
        _add(f"embed n{n} seq{seq} D{D} {mode}", "embed", n=n, seq=seq, V=V, D=D, mode=mode)
for C in (8, 72):
    for xf32 in (0, 1):
        _add(f"add_nchw C{C} {'f32' if xf32 else 'x16'} coded", "add", B=3, C=C, HW=100, xf32=xf32, kind="coded", pad=8)
        _add(f"add_nchw C{C} {'f32' if xf32 else 'x16'} slice of a wider row", "add", B=3, C=C, HW=67, xf32=xf32, kind="random", pad=40)
for n in (77, 300, _over("mask_to_bias", 77)):
    _add(f"mask_to_bias n{n}", "mask", n=n)


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def _canary(shape, ld, kind):
    """a [rows, C] or [B, HW, C] view with row stride ld in a flat canary buffer, 3 extra rows and 64 elements behind: (view, guard)"""
    g = KP.Guarded.rows(shape, ld, kind, extra_rows=3, tail=64, dt=_lib.elem_dtype())
    return g.view, g


_nan_rows = functools.partial(KP.nan_rows, tail=64)   # (vals [..., C], ld) -> a view with row stride ld in a NaN buffer, 64 NaN behind


def _flat_in(vals):
    """a flat floating-point input followed by NaN (an empty input: a valid pointer to NaN alone)"""
    if vals.numel() == 0:
        return torch.full((64,), float("nan"), dtype=vals.dtype, device="cuda")
    return _nan_rows(vals.reshape(1, -1), vals.numel())[0]


def _flat_out(n, kind):
    view, g = _canary((1, n), n, kind)
    return view[0], g


def _tally(res, g):
    uw, ow = g.counts()
    res["unwritten"] = res.get("unwritten", 0) + uw
    res["overwritten"] = res.get("overwritten", 0) + ow


def _randn(shape, g, scale=1.0):
    return scale * torch.randn(shape, generator=g, device="cuda")


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def run_case(name):
    fam, s = CASES[name]
    lib = _lib.load()
    ed = _lib.elem_dtype()
    st = ops._stream()
    g = torch.Generator(device="cuda").manual_seed(sum(map(ord, name)))
    res = {"unwritten": 0, "overwritten": 0}
    if fam == "silu":
        idt, odt = (F32 if s["in_f32"] else ed), (F32 if s["out_f32"] else ed)
        if s["n"] == "sweep":
            vals = RB.sweep32(ed, "cuda") if s["in_f32"] else RB.sweep16(ed, "cuda")
            if s["in_f32"] and s["out_f32"]:
                big = torch.finfo(F32).max
                vals = torch.cat([vals, torch.tensor([big, -big], device="cuda")])
        else:
            vals = _randn(s["n"], g, 4.0).to(idt)
        x = _flat_in(vals)
        if s["n"] == "sweep" and idt == odt:   # the wrapper's own path (same dtype in and out); its output has no canary
            y0 = ops.silu(x.clone())
        y, bits = _flat_out(vals.numel(), 32 if s["out_f32"] else 16)
        res["rc"] = lib.mi355x_sd_silu(x.data_ptr(), y.data_ptr(), vals.numel(), s["in_f32"], s["out_f32"], st)
        torch.cuda.synchronize()
        ref, e = RB.act("silu", vals.double())
        res["ratio"] = RB.check(y, ref, e)
        if s["n"] == "sweep" and idt == odt:
            res["wrapper_off"] = RB.exact_off(y0, y.clone())
        _tally(res, bits)
    elif fam == "act":
        vals = RB.sweep16(ed, "cuda") if s["n"] == "sweep" else _randn(s["n"], g, 3.0).to(ed)
        x = _flat_in(vals)
        y, bits = _flat_out(vals.numel(), 16)
        res["rc"] = lib.mi355x_sd_activation(x.data_ptr(), y.data_ptr(), vals.numel(), RB.KINDS[s["kind"]], st)
        torch.cuda.synchronize()
        ref, e = RB.act(s["kind"], vals.double())
        res["ratio"] = RB.check(y, ref, e)
        _tally(res, bits)
    elif fam == "gated":
        F = s["F"]
        if s["rows"] == "sweep":
            a = RB.sweep16(ed, "cuda")
            a = torch.cat([a, torch.zeros((-a.numel()) % F, dtype=ed, device="cuda")]).reshape(-1, F)
            b = _randn(a.shape, g, 2.0)
            b = torch.where(a.float().abs() > 128.0, torch.full_like(b, -0.5), b).to(ed)   # (the product stays finite)
        else:
            a, b = _randn((s["rows"], F), g, 3.0).to(ed), _randn((s["rows"], F), g, 2.0).to(ed)
        rows = a.shape[0]
        x = _nan_rows(torch.cat([a, b], 1), 2 * F + s["xpad"])
        y, bits = _canary((rows, F), F + 8, 16)
        res["rc"] = lib.mi355x_sd_gated_activation(x.data_ptr(), x.stride(0), y.data_ptr(), F + 8, rows, F, RB.KINDS[s["kind"]], st)
        torch.cuda.synchronize()
        ref, e = RB.gated(s["kind"], a.double(), b.double())
        res["ratio"] = RB.check(y, ref, e)
        _tally(res, bits)
        if s["xpad"] == 0:   # the wrapper's compact call is the same launch
            res["wrapper_off"] = RB.exact_off(ops.gated_activation(x, s["kind"]), y.contiguous())
    elif fam == "softmax":
        vals = RB.softmax_rows_input(s["n"], "cuda")
        x = _nan_rows(vals, s["n"] + 12)
        y, bits = _canary(tuple(vals.shape), s["n"] + 8, 16)
        ops.softmax_rows(x, out=y)
        torch.cuda.synchronize()
        res["rc"] = 0
        ref, e = RB.softmax(vals)
        res["ratio"] = RB.check(y, ref, e)
        res["wrapper_off"] = RB.exact_off(ops.softmax_rows(vals), y.contiguous())   # compact rows: the same bits
        _tally(res, bits)
    elif fam == "temb":
        dim, group = s["dim"], s.get("group", 1)
        t = torch.tensor(s.get("t", TS), dtype=F32, device="cuda")
        n = s.get("n", t.numel())
        ldo = group * dim + (8 if group == 1 else 40)
        y, bits = _canary((n // group, group * dim), ldo, 16)
        tin = _flat_in(t)
        args = (s["flip"], s["shift"], s.get("scale", 1.0), s.get("period", 10000.0))
        res["rc"] = lib.mi355x_sd_timestep_embedding(tin.data_ptr(), t.numel(), n, dim, group, *args, y.data_ptr(), ldo, st)
        torch.cuda.synchronize()
        ref, e = RB.timestep(t, n, dim, *args)
        got = y.reshape(n, dim)
        res["ratio"] = RB.check(got, ref, e)
        if dim & 1:
            res["pad_off"] = int((got[:, dim - 1].contiguous().view(torch.int16) != 0).sum().item())
        if group == 1 and t.numel() == n:   # the wrapper's compact call
            res["wrapper_off"] = RB.exact_off(ops.timestep_embedding(t, dim, bool(s["flip"]), s["shift"], s.get("scale", 1.0),
                                                                     s.get("period", 10000.0)), got.contiguous())
        _tally(res, bits)
    elif fam in ("axpby", "cfg"):
        n = s["n"]
        coef = _flat_in(torch.tensor(s["coef"], dtype=F32, device="cuda"))
        xv = _randn(n, g, 3.0)
        if fam == "axpby":
            yv = xv * (1 + 2.0 ** -12 * _randn(n, g)) if s["kind"] == "cancel" else _randn(n, g)
            yin = _flat_in(yv)
            out, bits = _flat_out(n, 32)
            if s["alias"]:   # out = x, as the benchmark's denoising loop updates its latents
                out.copy_(xv)
                xin = out
            else:
                xin = _flat_in(xv)
            res["rc"] = lib.mi355x_sd_axpby(xin.data_ptr(), yin.data_ptr(), out.data_ptr(), coef.data_ptr(), n, st)
            ref, e = RB.axpby(xv, yv, coef)
        else:   # eps_uncond / eps_text are the two halves of one tensor and out is a fresh one, as pipeline.py calls it
            uv = _randn(n, g)
            tv = uv * (1 + 2.0 ** -10 * _randn(n, g)) if s["gs"] == 1.0 else uv + 0.3 * _randn(n, g)
            if s["gs"] == 0.0:
                uv = xv * (1 + 2.0 ** -12 * _randn(n, g))   # coefficients of opposite sign, cancelling operands
            both = _flat_in(torch.cat([uv, tv]))
            xin = _flat_in(xv)
            out, bits = _flat_out(n, 32)
            res["rc"] = lib.mi355x_sd_cfg_axpby(xin.data_ptr(), both.data_ptr(), both.data_ptr() + 4 * n, out.data_ptr(),
                                                coef.data_ptr(), s["gs"], n, st)
            ref, e = RB.cfg_axpby(xv, uv, tv, coef, s["gs"])
        torch.cuda.synchronize()
        res["ratio"] = RB.check(out, ref, e)
        _tally(res, bits)
    elif fam == "latent":
        B, L, HW = s["B"], s["L"], s["HW"]
        mv = torch.cat([_randn((B * HW, L), g, 3.0), _randn((B * HW, L), g, 20.0)], 1)
        mv[0, L:] = torch.tensor([-30.0, 20.0, -30.5, 20.5][:L], device="cuda")
        mv[1, 0] = -0.0
        m = _nan_rows(mv, 2 * L + 4)
        nv = _randn((B, L, HW), g)
        outs = [_canary((B * L, HW), HW, 32) for _ in range(3)]
        noise = _flat_in(nv) if s["noise"] else None
        res["rc"] = lib.mi355x_sd_latent_dist(m.data_ptr(), 2 * L + 4, B, L, HW, ops._p(noise), 0.18215, outs[0][0].data_ptr(),
                                              outs[1][0].data_ptr(), outs[2][0].data_ptr(), st)
        torch.cuda.synchronize()
        mean, lv, mode = RB.latent_moments(mv, B, L, 0.18215)
        got = [o[0].reshape(B, L, HW) for o in outs]
        res["off"] = RB.exact_off(got[0], mean) + RB.exact_off(got[1], lv)
        if s["noise"]:
            res["ratio"] = RB.check(got[2], *RB.latent_sample(mv, B, L, nv, 0.18215))
        else:
            res["off"] += RB.exact_off(got[2], mode)
        for _, bits in outs:
            _tally(res, bits)
    elif fam in ("copy", "cast"):
        rows, C = s["rows"], s["C"]
        if fam == "copy":
            vals = RB.codes(rows * C, ed, "cuda").reshape(rows, C)
        else:
            vals = _randn((rows, C), g, 3.0) * 2.0 ** torch.randint(-30, 18, (rows, C), generator=g, device="cuda").float()
            vals[0, :8] = torch.tensor([float("inf"), -float("inf"), 3.4e38, 65520.0, 65519.9, 2.0 ** -25, 1.5 * 2.0 ** -24, -0.0],
                                       device="cuda")
        x = _nan_rows(vals, C + 16)
        y, bits = _canary((rows, C), C + 8, 16)
        fn = lib.mi355x_sd_copy_rows if fam == "copy" else lib.mi355x_sd_cast_rows
        res["rc"] = fn(x.data_ptr(), C + 16, y.data_ptr(), C + 8, rows, C, st)
        torch.cuda.synchronize()
        res["off"] = RB.exact_off(y, vals.to(ed))
        _tally(res, bits)
    elif fam == "patchify":
        B, C, H, W, p = s["B"], s["C"], s["H"], s["W"], s["p"]
        K, rows = C * p * p, B * (H // p) * (W // p)
        xv = RB.codes(B * C * H * W, ed, "cuda").float().reshape(B, C, H, W)
        x = _flat_in(xv).reshape(B, C, H, W)
        y, bits = _canary((rows, K), K + s["pad"], 16)
        res["rc"] = lib.mi355x_sd_patchify(x.data_ptr(), B, C, H, W, p, y.data_ptr(), K + s["pad"], st)
        torch.cuda.synchronize()
        res["off"] = RB.exact_off(y, RB.patchify(xv, p, ed))
        if s["pad"] == 0:
            res["wrapper_off"] = RB.exact_off(ops.patchify(xv, p), y.contiguous())
        _tally(res, bits)
    elif fam == "unpatchify":
        B, C, H, W, p = s["B"], s["C"], s["H"], s["W"], s["p"]
        K, rows = C * p * p, B * (H // p) * (W // p)
        xv = RB.codes(rows * K, ed, "cuda").reshape(rows, K)
        x = _nan_rows(xv, K + s["pad"])
        y, bits = _flat_out(B * C * H * W, 32)
        res["rc"] = lib.mi355x_sd_unpatchify(x.data_ptr(), K + s["pad"], B, C, H, W, p, y.data_ptr(), st)
        torch.cuda.synchronize()
        want = RB.unpatchify(xv, B, C, H, W, p)
        res["off"] = RB.exact_off(y.reshape(B, C, H, W), want)
        res["wrapper_off"] = RB.exact_off(ops.unpatchify(x, B, C, H, W, p), want)
        _tally(res, bits)
    elif fam == "split":
        B, S1, S2, C = s["B"], s["S1"], s["S2"], s["C"]
        allv = RB.codes(B * (S1 + S2) * 3 * C, ed, "cuda")
        xv, yv = allv[:B * S1 * 3 * C].reshape(B, S1, 3 * C), allv[B * S1 * 3 * C:].reshape(B, S2, 3 * C)
        x, y = _flat_in(xv), _flat_in(yv)
        outs = [_canary((B * (S1 + S2), C), C, 16) for _ in range(3)]
        res["rc"] = lib.mi355x_sd_split_concat(x.data_ptr(), y.data_ptr(), *(o[0].data_ptr() for o in outs), B, S1, S2, C, st)
        torch.cuda.synchronize()
        want = RB.split_concat(xv, yv)
        res["off"] = sum(RB.exact_off(o[0].reshape(B, S1 + S2, C), w) for o, w in zip(outs, want))
        if S1 and S2:
            res["wrapper_off"] = sum(RB.exact_off(a, w) for a, w in zip(ops.split_concat(xv, yv), want))
        for _, bits in outs:
            _tally(res, bits)
    elif fam == "embed":
        n, seq, V, D = s["n"], s["seq"], s["V"], s["D"]
        ids = torch.randint(0, V, (n,), generator=g, device="cuda").to(torch.int32)
        ids[0], ids[-1], ids[n // 2] = 0, V - 1, V - 1
        tok = RB.codes(V * D, ed, "cuda").reshape(V, D)
        pos = RB.codes(seq * D, ed, "cuda").flip(0).reshape(seq, D)
        if s["mode"] == "tok+pos":   # (values whose sum rounds)
            tok, pos = _randn((V, D), g).to(ed), _randn((seq, D), g, 0.1).to(ed)
            tok[0, :4] = torch.tensor([-0.0, 0.0, -0.0, 1.0], device="cuda").to(ed)
        elif s["mode"] == "pos":
            tok = torch.zeros_like(tok)
        if s["mode"] == "tok":
            tok[0, 0] = -0.0   # float(-0) + 0 = +0
        tk = _nan_rows(tok, D)
        ps = _nan_rows(pos, D) if s["mode"] != "tok" else None
        y, bits = _canary((n, D), D + 8, 16)
        res["rc"] = lib.mi355x_sd_embed_tokens(ids.data_ptr(), n, seq, tk.data_ptr(), ops._p(ps), D, y.data_ptr(), D + 8, st)
        torch.cuda.synchronize()
        want = RB.embed_tokens(ids, tok, pos if ps is not None else None, seq)
        res["off"] = RB.exact_off(y, want)
        if ps is not None:
            res["wrapper_off"] = RB.exact_off(ops.embed_tokens(ids, tk, ps, seq), want)
        _tally(res, bits)
    elif fam == "add":
        B, C, HW, xf32 = s["B"], s["C"], s["HW"], s["xf32"]
        xdt = F32 if xf32 else ed
        if s["kind"] == "coded":   # x = 0: the output IS the residual's code
            xv = torch.zeros((B, HW, C), device="cuda", dtype=xdt)
            rv = RB.codes(B * C * HW, ed, "cuda").float().reshape(B, C, HW)
        else:
            xv, rv = _randn((B, HW, C), g, 3.0).to(xdt), _randn((B, C, HW), g)
        x, bits = _canary((B, HW, C), C + s["pad"], 32 if xf32 else 16)
        x.copy_(xv)
        r = _flat_in(rv)
        res["rc"] = lib.mi355x_sd_add_nchw_ex(x.data_ptr(), C + s["pad"], r.data_ptr(), B, C, HW, xf32, st)
        torch.cuda.synchronize()
        res["off"] = RB.exact_off(x, RB.add_nchw(xv, rv))
        _tally(res, bits)
    elif fam == "mask":
        n = s["n"]
        mv = (torch.rand(n, generator=g, device="cuda") < 0.5).float()
        mv[:8] = torch.tensor([0.0, 1.0, 0.5, 0.3, -0.0, 1e-8, 0.999999, 2.0], device="cuda")
        m = _flat_in(mv)
        y, bits = _flat_out(n, 32)
        res["rc"] = lib.mi355x_sd_mask_to_bias(m.data_ptr(), y.data_ptr(), n, st)
        torch.cuda.synchronize()
        res["off"] = RB.exact_off(y, RB.mask_to_bias(mv))
        _tally(res, bits)
    return res


def _case_or_error(name):
    try:
        return run_case(name)
    except (ValueError, TypeError, IndexError, ZeroDivisionError, AssertionError, _lib.MI355XError) as ex:
        # a refusal or a mistake of the case's own host code: reported as that case's failure (a device error ends the child)
        return {"error": f"{type(ex).__name__}: {ex}"}


if __name__ == "__main__":
    KP.run_cases(CASES, _case_or_error, route_log=None, tag="ROWMAP_JSON", names=sys.argv[1:])
