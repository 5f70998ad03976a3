"""Child of tests/test_gpu_gemm_f8.py: the case matrix of the W8A8 GEMM -- gemm256_kernel<false, false, true> (csrc/gemm256.hip) with
gemm_epilogue_f8 (csrc/gemm_epilogue.h), the only kernel launch_gemm_f8 has, so there is no route to log -- through the C entries
mi355x_sd_linear_f8 / mi355x_sd_linear_f8_q themselves, which is where the row remaps and the strides can be reached. References,
bounds and operand generators: tests/gemm_f8_bounds.py. Prints one JSON line.

  python tests/gemm_f8_child.py [case ...]     (no names: every case)

Buffers. A and W are e4m3 bytes; the row gaps of A (lda = K + 16), the rows of the other segment under the A remap and the space after
the last row of A and of W hold 0x7F, NaN in e4m3fn: a stray read poisons the output. a_scale, w_scale, bias, the gate (ld_gate = N +
8: in its row gaps too) and a_l2 are followed by NaN; the residual's row gaps (ldr = N + 12) hold NaN. The 16-bit output is a view
with ldc = N + 8 inside a buffer of the 0x7FA5 canary, the e4m3 output one with ldc % 8 == 0 inside a buffer of 0x7F (never a result:
finite inputs saturate to 448), c_scale sits in a 0x7FA5A5A5 buffer with spare entries; under the C remap the rows of the other
segment are canary too. Every case reports `unwritten` and `overwritten`. Every launch without an A remap is repeated through the
ops.linear_f8 / ops.linear_f8_q wrapper on compact operands (linear_f8_q: where N % 8 == 0, its output has ldc = N): `wrapper_off`
counts the differing bits.

Class 1 ("x ..."): exact bits, `off`. Class 2 ("d ...", "q ..."): the float64 bound, `ratio` / `rel`, and the interval rule of the
e4m3 output. Refusals ("refuse ..."): a non-zero status and an untouched canary.

Shapes: the smallest that reach each edge of the 256 x 256 tile with its 128-element K-tile, 16-row and 32-column sub-tiles -- M in
{1, 16, 77, 255, 256, 257} x N in {4, 12, 252, 256, 260} at one K-tile (the prologue's second tile entirely run-out; N = 12 and 260
end on the 4-wide store), two and three K-tiles (both buffer parities, an odd count), 3 x 3 ragged tiles, 9 x 4 tiles (more row
tiles than gemm_gm() groups, a tile count that is no multiple of 8: xcd_remap), K = 1536 and the model's deepest, 6144; segments of
77 and 40 rows inside batches of 117 for both remaps, the second launched from a base pointer at row 77 as sd3.py does."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import kernel_pieces as KP  # noqa: E402

SEG = (77, 40)         # the two segments of a joint buffer's batch
BATCH_ROWS = sum(SEG)  # 117
NBATCH = 3

CASES = {}


def _add(name, **spec):
    assert name not in CASES
    CASES[name] = spec


# ---- class 1 -----------------------------------------------------------------------------------------------------------------------
for _mir in ("As", "Ws"):
    _shapes = [(M, N, 128) for M in (1, 16, 77, 255, 256, 257) for N in (4, 12, 252, 256, 260)]
    _shapes += [(257, 260, 256), (257, 260, 384), (600, 520, 256), (2300, 780, 128), (300, 264, 1536), (300, 264, 6144)]
    for _M, _N, _K in _shapes:
        _add(f"x {_mir} {_M}x{_N}x{_K} scale", cls="exact", mirror=_mir, sub="scale", M=_M, N=_N, K=_K, q=True)
    _add(f"x {_mir} 231x260x256 epi", cls="exact", mirror=_mir, sub="epi", M=231, N=260, K=256)
    for _i, _seg in enumerate(SEG):
        _add(f"x {_mir} a-remap {_seg}", cls="exact", mirror=_mir, sub="scale", M=NBATCH * _seg, N=260, K=256, a_seg=_i)
        _add(f"x {_mir} c-remap {_seg}", cls="exact", mirror=_mir, sub="scale", M=NBATCH * _seg, N=260, K=256, c_seg=_i)

# ---- class 2 -----------------------------------------------------------------------------------------------------------------------
for _M, _N, _K in ((257, 328, 256), (515, 324, 384), (231, 648, 128), (300, 264, 6144)):
    for _form in ("", "bias", "bias+gelu", "gate", "gate+gelu"):
        _add(f"d {_M}x{_N}x{_K} {_form or 'nobias'}", cls="dense", M=_M, N=_N, K=_K, form=_form)
    _add(f"d {_M}x{_N}x{_K} c-remap", cls="dense", M=_M, N=_N, K=_K, form="bias", c_rpb=77)
for _M, _N, _K, _ldc in ((300, 520, 256, 528), (77, 8, 128, 16), (257, 12, 128, 16), (515, 6144, 128, 6152)):
    for _gelu in (False, True):
        _add(f"q {_M}x{_N}x{_K}{' gelu' if _gelu else ''}", cls="denseq", M=_M, N=_N, K=_K, form="bias+gelu" if _gelu else "bias",
             ldc=_ldc)

# ---- refusals ------------------------------------------------------------------------------------------------------------------------
for _what in ("K%128", "N%4", "lda%16", "ldc%4", "q ldc%8", "gate rpb0", "a_bstride%16", "c_bstride%4", "ldr%4", "flag"):
    _add(f"refuse {_what}", cls="refuse", what=_what)


# ---- buffers -----------------------------------------------------------------------------------------------------------------------
def _bytes_rows(q, ld, rpb=0, bstride=0, base=0, total_rows=None):
    """q [M, C] e4m3 bytes placed row by row (tests/gemm_f8_bounds.row_offsets) in a flat buffer of 0x7F, 256 more bytes behind"""
    import torch
    from tests import gemm_f8_bounds as FB
    M, C = q.shape
    rows = total_rows if total_rows is not None else M
    buf = torch.full((rows * ld + 256,), FB.F8_NAN, dtype=torch.uint8, device="cuda")
    idx = base + FB.row_offsets(M, ld, rpb, bstride, "cuda")[:, None] + torch.arange(C, device="cuda")
    buf[idx] = q.cuda()
    return buf


def _vec_nan(v):
    """fp32 vector followed by 64 NaN"""
    return KP.nan_rows(v.cuda().float().reshape(1, -1), v.numel(), tail=64)[0]


def _rows_nan(vals, ld):
    """[R, C] values as a view with row stride ld inside a NaN buffer, 64 NaN behind"""
    return KP.nan_rows(vals.cuda(), ld, tail=64)


def _out(M, N, ld, kind, ed=None, rpb=0, bstride=0, base=0, total_rows=None):
    """an [M, N] output placed row by row (tests/gemm_f8_bounds.row_offsets) in a flat canary buffer with 3 more rows and 64 more
    elements: 16-bit (0x7FA5), e4m3 bytes (0x7F) or fp32 (0x7FA5A5A5)"""
    import torch
    from tests import gemm_f8_bounds as FB
    rows = (total_rows if total_rows is not None else M) + 3
    idx = base + FB.row_offsets(M, ld, rpb, bstride, "cuda")[:, None] + torch.arange(N, device="cuda")
    return KP.Guarded.at(idx, rows * ld + 64, kind, base=base, dt=ed, canary=KP.F8_NAN if kind == 8 else None)


# ---- one launch of each entry ----------------------------------------------------------------------------------------------------
def _run16(o, ed, M, N, K, *, a_seg=None, c_seg=None, c_rpb=0):
    """mi355x_sd_linear_f8 on the operands o -> (result dict, output [M, N])"""
    import torch
    from tests.bound_pieces import exact_off
    from paddlemix_amd import _lib, ops
    lib, st = _lib.load(), ops._stream()
    lda, ldc = K + 16, N + 8
    a_rpb = a_bs = a_base = 0
    if a_seg is not None:   # this launch's segment of every batch; the other segment's rows stay 0x7F
        a_rpb, a_bs, a_base = SEG[a_seg], BATCH_ROWS * lda, (SEG[0] * lda if a_seg else 0)
    A = _bytes_rows(o["qa"], lda, a_rpb, a_bs, a_base, total_rows=NBATCH * BATCH_ROWS if a_seg is not None else None)
    W = _bytes_rows(o["qw"], K)
    sa, sw = _vec_nan(o["sa"]), _vec_nan(o["sw"])
    bias = _vec_nan(o["bias"]) if o["bias"] is not None else None
    gate = _rows_nan(o["gate"].float(), N + 8) if o["gate"] is not None else None
    res = _rows_nan(o["residual"], N + 12) if o["residual"] is not None else None
    c_bs = c_base = 0
    total = None
    if c_seg is not None:
        c_rpb, c_bs, c_base, total = SEG[c_seg], BATCH_ROWS * ldc, (SEG[0] * ldc if c_seg else 0), NBATCH * BATCH_ROWS
    elif c_rpb:             # batches of c_rpb rows written behind 40 other rows each
        c_bs, total = (c_rpb + 40) * ldc, ((M + c_rpb - 1) // c_rpb) * (c_rpb + 40)
    out = _out(M, N, ldc, 16, ed, c_rpb, c_bs, c_base, total)
    flags = _lib.GELU_TANH if o.get("gelu") else 0
    rc = lib.mi355x_sd_linear_f8(A.data_ptr() + a_base, lda, a_rpb, a_bs, sa.data_ptr(), W.data_ptr(), sw.data_ptr(), out.ptr, ldc,
                                 c_rpb, c_bs, M, N, K, ops._p(bias), ops._p(gate), N + 8 if gate is not None else 0, o["rpb"],
                                 ops._p(res), N + 12 if res is not None else 0, flags, st)
    torch.cuda.synchronize()
    got = out.get()
    r = dict(rc=rc)
    r["unwritten"], r["overwritten"] = out.counts()
    if a_seg is None:       # the wrapper's compact call is the same launch
        w = ops.linear_f8(o["qa"].cuda(), sa, o["qw"].cuda(), sw, bias, gate=None if gate is None else gate.contiguous(),
                          rows_per_batch=o["rpb"], residual=None if res is None else res.contiguous(), gelu_tanh=bool(o.get("gelu")))
        torch.cuda.synchronize()
        r["wrapper_off"] = exact_off(w, got)
    return r, got


def _run8(o, M, N, K, ldc):
    """mi355x_sd_linear_f8_q on the operands o -> (result dict, bytes [M, N], c_scale [M])"""
    import torch
    from tests.bound_pieces import exact_off
    from paddlemix_amd import _lib, ops
    lib, st = _lib.load(), ops._stream()
    lda = K + 16
    A, W = _bytes_rows(o["qa"], lda), _bytes_rows(o["qw"], K)
    sa, sw, l2 = _vec_nan(o["sa"]), _vec_nan(o["sw"]), _vec_nan(o["a_l2"])
    bias = _vec_nan(o["bias"]) if o["bias"] is not None else None
    out = _out(M, N, ldc, 8)
    cs = _out(M, 1, 1, 32, total_rows=M + 8)
    flags = _lib.GELU_TANH if o.get("gelu") else 0
    rc = lib.mi355x_sd_linear_f8_q(A.data_ptr(), lda, sa.data_ptr(), l2.data_ptr(), W.data_ptr(), sw.data_ptr(), o["w_norm_max"],
                                   out.ptr, ldc, cs.ptr, M, N, K, ops._p(bias), o["bias_abs_max"], flags, st)
    torch.cuda.synchronize()
    q, c = out.get(), cs.get()[:, 0]
    r = dict(rc=rc)
    r["overwritten"] = out.counts()[1] + cs.counts()[1]
    r["unwritten"] = cs.counts()[0]   # (an unwritten output byte is a NaN byte: counted by check_q)
    if N % 8 == 0:   # the wrapper's compact output has ldc = N: the e4m3 store needs ldc % 8 == 0
        wq, wc = ops.linear_f8_q(o["qa"].cuda(), sa, l2, o["qw"].cuda(), sw, o["w_norm_max"], bias, o["bias_abs_max"],
                                 gelu_tanh=bool(o.get("gelu")))
        torch.cuda.synchronize()
        r["wrapper_off"] = exact_off(wq, q) + exact_off(wc, c)
    return r, q, c


def _dev(o):
    import torch
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in o.items()}


def _check_q(r, o, q, c, ref, e):
    from tests import gemm_f8_bounds as FB
    s64 = FB.out_scale64(o["a_l2"], o["w_norm_max"], o["bias_abs_max"])
    r.update(FB.check_q(q, c, ref, e, s64))


def run_exact(s, ed):
    import torch
    from tests import gemm_bounds as GB
    from tests import gemm_f8_bounds as FB
    M, N, K = s["M"], s["N"], s["K"]
    o = FB.exact_operands(M, N, K, s["mirror"], s["sub"], ed)
    d = _dev(o)
    ref = FB.exact_reference(d, ed)   # (asserts the precondition)
    r, got = _run16(o, ed, M, N, K, a_seg=s.get("a_seg"), c_seg=s.get("c_seg"))
    r["off"] = FB.exact_off(got, ref)
    r["ratio"], r["rel"] = GB.check(got, ref, torch.zeros_like(ref))
    if s.get("q"):   # the same operands through the e4m3 output, judged by the interval rule
        FB.exact_q_operands(o)
        _, e = FB.reference8(d["qa"], d["sa"], d["qw"], d["sw"])
        rq, q, c = _run8(o, M, N, K, (N + 8 + 7) // 8 * 8)
        _check_q(rq, _dev(o), q, c, ref, e)
        r["q"] = rq
    return r


def run_dense(s, ed):
    from tests import gemm_bounds as GB
    from tests import gemm_f8_bounds as FB
    M, N, K = s["M"], s["N"], s["K"]
    o = FB.dense_operands(M, N, K, s["form"], ed)
    d = _dev(o)
    ref, e = FB.reference8(d["qa"], d["sa"], d["qw"], d["sw"], bias=d["bias"], gate=d["gate"], rows_per_batch=d["rpb"],
                           residual=d["residual"], gelu=d["gelu"])
    if s["cls"] == "denseq":
        r, q, c = _run8(o, M, N, K, s["ldc"])
        _check_q(r, d, q, c, ref, e)
        return r
    r, got = _run16(o, ed, M, N, K, c_rpb=s.get("c_rpb", 0))
    r["ratio"], r["rel"] = GB.check(got, ref, e)
    return r


def run_refusal(s, ed):
    """one broken argument of an otherwise valid 32 x 8 x 128 launch -> the status, and how much of the canary changed"""
    import torch
    from paddlemix_amd import _lib, ops
    from tests.kernel_pieces import CANARY16, CANARY32, F8_NAN
    lib, st = _lib.load(), ops._stream()
    what = s["what"]
    M, N, K = 32, 8, 128
    a = dict(lda=K + 16, a_rpb=0, a_bs=0, ldc=N + 8, c_rpb=0, c_bs=0, M=M, N=N, K=K, gate=False, rpb=0, res=False, ldr=0, flags=0)
    q8 = what == "q ldc%8"
    if what == "K%128":
        a["K"] = 64
    elif what == "N%4":
        a["N"] = 6
    elif what == "lda%16":
        a["lda"] = K + 8
    elif what == "ldc%4":
        a["ldc"] = N + 2
    elif q8:
        a["ldc"] = N + 4
    elif what == "gate rpb0":
        a.update(gate=True, rpb=0)
    elif what == "a_bstride%16":
        a.update(a_rpb=16, a_bs=16 * a["lda"] + 8)
    elif what == "c_bstride%4":
        a.update(c_rpb=16, c_bs=16 * a["ldc"] + 2)
    elif what == "ldr%4":
        a.update(res=True, ldr=N + 2)
    elif what == "flag":
        a["flags"] = _lib.SILU
    else:
        raise ValueError(what)
    A = torch.full((4 * M * (K + 16),), 0x38, dtype=torch.uint8, device="cuda")   # (1.0 everywhere: were it launched, it would write)
    W = torch.full((4 * N * K,), 0x38, dtype=torch.uint8, device="cuda")
    ones = torch.ones(256, device="cuda")
    gate = torch.ones(4 * 64, device="cuda")
    res = torch.ones(4 * M * 64, device="cuda").to(ed)
    if q8:
        bits = torch.full((4 * M * 64,), F8_NAN, dtype=torch.uint8, device="cuda")
        cs = torch.full((M + 8,), CANARY32, dtype=torch.int32, device="cuda")
        rc = lib.mi355x_sd_linear_f8_q(A.data_ptr(), a["lda"], ones.data_ptr(), ones.data_ptr(), W.data_ptr(), ones.data_ptr(), 1.0,
                                       bits.data_ptr(), a["ldc"], cs.data_ptr(), M, a["N"], a["K"], None, 0.0, 0, st)
        torch.cuda.synchronize()
        return dict(rc=rc, overwritten=int((bits != F8_NAN).sum().item()) + int((cs != CANARY32).sum().item()))
    bits = torch.full((4 * M * 64,), CANARY16, dtype=torch.int16, device="cuda")
    rc = lib.mi355x_sd_linear_f8(A.data_ptr(), a["lda"], a["a_rpb"], a["a_bs"], ones.data_ptr(), W.data_ptr(), ones.data_ptr(),
                                 bits.data_ptr(), a["ldc"], a["c_rpb"], a["c_bs"], M, a["N"], a["K"], None,
                                 gate.data_ptr() if a["gate"] else None, 8 if a["gate"] else 0, a["rpb"],
                                 res.data_ptr() if a["res"] else None, a["ldr"], a["flags"], st)
    torch.cuda.synchronize()
    r = dict(rc=rc, overwritten=int((bits != CANARY16).sum().item()))
    if what == "K%128":   # through the wrapper: MI355XError
        try:
            ops.linear_f8(A[:M * 64].view(M, 64), ones[:M], W[:N * 64].view(N, 64), ones[:N])
            r["wrapper_raises"] = False
        except _lib.MI355XError:
            r["wrapper_raises"] = True
    return r


def run_case(name):
    from paddlemix_amd import _lib
    s = CASES[name]
    return {"exact": run_exact, "dense": run_dense, "denseq": run_dense, "refuse": run_refusal}[s["cls"]](s, _lib.elem_dtype())


if __name__ == "__main__":
    KP.run_cases(CASES, run_case, route_log=None, tag="F8_JSON", names=sys.argv[1:])
