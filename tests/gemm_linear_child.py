"""Child of tests/test_gpu_gemm_linear.py: the case matrix of the 16-bit linear GEMM kernel families -- the generic loop of
csrc/gemm.hip on its four tiles (and its e4m3-weight and LayerNorm-fold instantiations), split-K slices + splitk_reduce_kernel, the
pipelined loops of csrc/gemm_pipe.hip with the early-residual kernel, the phased 256 x 256 kernel of csrc/gemm256.hip, the small tile
of csrc/gemm_small.hip -- under the MI355X_SD_* switches of its environment (read once per process). Every case is held to the
elementwise float64 bound of tests/gemm_bounds.py over its WHOLE output; with MI355X_SD_GEMM_LOG set (debug build) each case also
reports the kernel family dispatch_gemm logged for it. Prints one JSON line: per case sha256 of the output, worst err / bound,
rel-L2, guard-band findings, route.

  python tests/gemm_linear_child.py [case ...]     (no names: every case that is not tied to one switch set)

The shapes are the smallest that reach each path: 1, 2, 3, 5 and 7 K-tiles (prologue and tail alone, both sides of the early-residual
kernel's TM + 2, past the small tile's six-stage ring), 35 K-tiles (split-K with an uneven last slice), K % 64 != 0; one to five row
tiles with 1 .. 3 live rows in the last; N = 4 .. 648 with N % 8 == 4 (the narrow store path). Batched operands use 77 and 154 rows
per batch, so a batch boundary falls inside a 16-row sub-tile and inside a tile."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import kernel_pieces as KP  # noqa: E402

EXTRA = 154       # rows of other data between the batches of a remapped operand

# ---- switch sets (debug-switch build) ----------------------------------------------------------------------------------------------
_G = {"MI355X_SD_NO_PIPE": "1", "MI355X_SD_NO_SPLITK": "1"}
SWITCHES = {
    # the generic double-buffered loop on each of its tiles, one chain over K
    "g128": dict(_G, MI355X_SD_GEMM_TILE="128"),
    "g160": dict(_G, MI355X_SD_GEMM_TILE="160"),
    "g256": dict(_G, MI355X_SD_GEMM_TILE="256", MI355X_SD_NO_W4="1"),
    "g320": dict(_G, MI355X_SD_GEMM_TILE="320"),
    "g128sk": {"MI355X_SD_GEMM_TILE": "128", "MI355X_SD_NO_PIPE": "1"},   # ... with split-K slices where plan_splitk gives them
    # the pipelined loops (and the phased kernel, id 257) on each tile
    "p128": {"MI355X_SD_GEMM_TILE": "128"},
    "p128ns": {"MI355X_SD_GEMM_TILE": "128", "MI355X_SD_NO_SPLITK": "1"},   # (the small tile's bit-exact reference)
    "p129": {"MI355X_SD_GEMM_TILE": "129"},
    "p160": {"MI355X_SD_GEMM_TILE": "160"},
    "p320": {"MI355X_SD_GEMM_TILE": "320"},
    "p256": {"MI355X_SD_GEMM_TILE": "256"},
    "p257": {"MI355X_SD_GEMM_TILE": "257"},
    "pick": {},   # the picker: every case here is small enough for the small tile where that applies
}
# bias after the sum, one chain over K: the bits of the tile's generic configuration (GENERIC_OF)
for _t in ("128", "129", "160", "320", "256"):
    SWITCHES[f"p{_t}nb"] = {"MI355X_SD_GEMM_TILE": _t, "MI355X_SD_GEMM_NO_BIAS_ACC": "1", "MI355X_SD_NO_SPLITK": "1"}
    SWITCHES[f"p{_t}one"] = {"MI355X_SD_GEMM_TILE": _t, "MI355X_SD_GEMM_PERSIST": "0"}   # one block per tile (the persistent cases only)
GENERIC_OF = {"p128nb": "g128", "p129nb": "g128", "p160nb": "g160", "p320nb": "g320", "p256nb": "g256"}

# ---- expected routes, written out from dispatch_gemm / launch_gemm_pipe / gemm_small_applies / plan_splitk --------------------------
# Route class of a case (CASES' last column):
#   plain    16-bit operands, K % 64 == 0, fewer than 8 K-tiles (plan_splitk: nt >= 8), no GEGLU, no A row remap
#   deep     the same at K = 2240 (35 K-tiles, <= 160 tiles): split-K slices under the 128 tile unless MI355X_SD_NO_SPLITK
#   k8       K % 64 != 0: launch_gemm_pipe, the phased kernel and the small tile refuse
#   geglu    GEGLU: the 160-wide tiles refuse (odd number of sub-tiles per wave) -> their launches end on the generic 128 tile
#   aremap   A row remap: the phased kernel refuses
#   ln, ln-deep, ln-geglu, ln-k8     the LayerNorm fold of the four classes above (128 x 160 refuses the fold)
#   f8, f8-deep                      e4m3 weight bytes read by the kernel: generic configurations only
_ALL = ("plain", "deep", "k8", "geglu", "aremap", "ln", "ln-deep", "ln-geglu", "ln-k8", "f8", "f8-deep")


def _generic(t, geglu_t=None, sk=False):
    """routes of a switch set that ends on the generic loop of tile t for every class (GEGLU on tile geglu_t)"""
    gt = geglu_t or t
    d = {c: f"generic/{t}" for c in ("plain", "deep", "k8", "aremap")}
    d.update({"geglu": f"generic/{gt}", "ln": f"generic/{t}+ln", "ln-deep": f"generic/{t}+ln", "ln-k8": f"generic/{t}+ln",
              "ln-geglu": f"generic/{gt}+ln", "f8": f"generic/{t}+f8", "f8-deep": f"generic/{t}+f8"})
    if sk:
        d.update({"deep": f"generic/{t}+splitk", "ln-deep": f"generic/{t}+ln+splitk", "f8-deep": f"generic/{t}+f8+splitk"})
    return d


ROUTES = {
    "g128": _generic(128), "g160": _generic(160, geglu_t=128), "g256": _generic(256), "g320": _generic(320),
    "g128sk": _generic(128, sk=True),
    "p128": {"plain": "pipe/128", "deep": "pipe/128+splitk", "k8": "generic/128", "geglu": "pipe/128", "aremap": "pipe/128",
             "ln": "pipe/128", "ln-deep": "pipe/128+splitk", "ln-geglu": "pipe/128", "ln-k8": "generic/128+ln",
             "f8": "generic/128+f8", "f8-deep": "generic/128+f8+splitk"},
    "p128ns": {"plain": "pipe/128", "deep": "pipe/128", "k8": "generic/128", "geglu": "pipe/128", "aremap": "pipe/128",
               "ln": "pipe/128", "ln-deep": "pipe/128", "ln-geglu": "pipe/128", "ln-k8": "generic/128+ln",
               "f8": "generic/128+f8", "f8-deep": "generic/128+f8"},
    "p129": {"plain": "pipe/129", "deep": "pipe/129", "k8": "generic/128", "geglu": "generic/128", "aremap": "pipe/129",
             "ln": "generic/128+ln", "ln-deep": "generic/128+ln", "ln-geglu": "generic/128+ln", "ln-k8": "generic/128+ln",
             "f8": "generic/128+f8", "f8-deep": "generic/128+f8"},
    "p160": {"plain": "pipe/160", "deep": "pipe/160", "k8": "generic/160", "geglu": "generic/128", "aremap": "pipe/160",
             "ln": "pipe/160", "ln-deep": "pipe/160", "ln-geglu": "generic/128+ln", "ln-k8": "generic/160+ln",
             "f8": "generic/160+f8", "f8-deep": "generic/160+f8"},
    "p320": {"plain": "pipe/320", "deep": "pipe/320", "k8": "generic/320", "geglu": "pipe/320", "aremap": "pipe/320",
             "ln": "pipe/320", "ln-deep": "pipe/320", "ln-geglu": "pipe/320", "ln-k8": "generic/320+ln",
             "f8": "generic/320+f8", "f8-deep": "generic/320+f8"},
    "p256": {"plain": "pipe/256", "deep": "pipe/256", "k8": "generic/256", "geglu": "pipe/256", "aremap": "pipe/256",
             "ln": "pipe/256", "ln-deep": "pipe/256", "ln-geglu": "pipe/256", "ln-k8": "generic/256+ln",
             "f8": "generic/256+f8", "f8-deep": "generic/256+f8"},
    "p257": {"plain": "gemm256", "deep": "gemm256", "k8": "generic/256", "geglu": "gemm256", "aremap": "generic/256",
             "ln": "gemm256+ln", "ln-deep": "gemm256+ln", "ln-geglu": "gemm256+ln", "ln-k8": "generic/256+ln",
             "f8": "generic/256+f8", "f8-deep": "generic/256+f8"},
    # the picker gives every one of these launches the 128 tile (at most 256 tiles of 128 x 128: one round, and two co-resident
    # blocks), then the small tile where gemm_small_applies holds: K % 64 == 0, no fp8 scale, <= 48 K-tiles
    "pick": {"plain": "small", "deep": "small", "k8": "generic/128", "geglu": "small", "aremap": "small",
             "ln": "small", "ln-deep": "small", "ln-geglu": "small", "ln-k8": "generic/128+ln",
             "f8": "generic/128+f8", "f8-deep": "generic/128+f8+splitk"},
}
for _t in ("128", "129", "160", "320", "256"):
    ROUTES[f"p{_t}nb"] = ROUTES["p128ns" if _t == "128" else f"p{_t}"]
    ROUTES[f"p{_t}one"] = ROUTES[f"p{_t}"]
assert all(set(r) == set(_ALL) for r in ROUTES.values()) and set(ROUTES) == set(SWITCHES)

# ---- cases -------------------------------------------------------------------------------------------------------------------------
# name: (M, N, K, kind, route class[, the switch sets it is tied to]). kind: plain | nobias | scale | silu | gelu (tanh, linear_ex) |
# geglu | R (bias + 16-bit residual) | R-nobias | Rwide (the residual a column slice of a wider buffer, ldr = N + 24) | R32 (fp32
# residual in, fp32 out) | rowbias:<rpb> | rowbias+R:<rpb> (+ out_scale) | rowbias+R32:<rpb> | gate+R:<rpb> | a-remap | c-remap (77
# rows per batch, EXTRA foreign rows between batches) | strided (lda = K + 64, out= a view with ldc = N + 16 inside a canary buffer
# with 40 spare rows) | ln | ln-nobias | ln-geglu | f8 | f8-nobias | f8-gelu | f8-gate+R:<rpb>
CASES = {
    # K: 1, 2, 3, 5, 7 K-tiles with a residual (the early-residual kernel needs TM + 2 = 6), 35, and K % 64 != 0
    "k64 R": (257, 328, 64, "R", "plain"),
    "k128 R": (257, 328, 128, "R", "plain"),
    "k192 R": (257, 328, 192, "R", "plain"),
    "k320 R": (257, 328, 320, "R", "plain"),
    "k448 R": (257, 328, 448, "R", "plain"),
    "k2240 R": (96, 640, 2240, "R", "deep"),
    "k2240 n324": (77, 324, 2240, "Rwide", "deep"),
    "k72": (257, 328, 72, "plain", "k8"),
    "k200 R": (77, 164, 200, "R", "k8"),
    # M: one row, one sub-tile + 1, 77, two row tiles of 256 + 3 (five of 128 + 3), a multiple of every tile
    "m1": (1, 328, 192, "plain", "plain"),
    "m17": (17, 36, 192, "plain", "plain"),
    "m77 silu": (77, 328, 128, "silu", "plain"),
    "m515": (515, 648, 192, "plain", "plain"),
    "m512 nobias": (512, 640, 128, "nobias", "plain"),
    # N: one channel group, N % 8 == 4 (narrow stores; the early fetch refuses), ragged against 128 / 160 / 256 / 320
    "n4": (17, 4, 64, "plain", "plain"),
    "n36 scale": (257, 36, 128, "scale", "plain"),
    "n164 R": (257, 164, 448, "R", "plain"),
    "n324 Rwide": (515, 324, 448, "Rwide", "plain"),
    "n648 Rwide": (257, 648, 448, "Rwide", "plain"),
    "geglu n352": (257, 352, 192, "geglu", "geglu"),
    "geglu k448 m77": (77, 352, 448, "geglu", "geglu"),
    # epilogue operands
    "gelu": (257, 328, 192, "gelu", "plain"),
    "R nobias": (257, 328, 448, "R-nobias", "plain"),
    "R32": (257, 328, 448, "R32", "plain"),
    "R32 n324": (77, 324, 128, "R32", "plain"),
    "rowbias 77": (231, 328, 192, "rowbias:77", "plain"),
    "rowbias 154 +R": (308, 164, 448, "rowbias+R:154", "plain"),
    "rowbias 77 +R32": (231, 328, 128, "rowbias+R32:77", "plain"),
    "gate+R 77": (231, 328, 192, "gate+R:77", "plain"),
    "gate+R 154": (308, 648, 448, "gate+R:154", "plain"),
    "a-remap": (231, 328, 192, "a-remap", "aremap"),
    "c-remap": (231, 328, 192, "c-remap", "plain"),
    "strided n324": (257, 324, 192, "strided", "plain"),
    "strided n328": (515, 328, 448, "strided", "plain"),
    # LayerNorm fold
    "ln": (257, 328, 192, "ln", "ln"),
    "ln nobias m77": (77, 164, 128, "ln-nobias", "ln"),
    "ln geglu": (515, 352, 448, "ln-geglu", "ln-geglu"),
    "ln k2240": (96, 648, 2240, "ln", "ln-deep"),
    "ln k72": (257, 328, 72, "ln", "ln-k8"),
    # e4m3 weight bytes read inside the generic loop (M < 4096: no widening pass)
    "f8": (257, 328, 192, "f8", "f8"),
    "f8 nobias": (17, 36, 64, "f8-nobias", "f8"),
    "f8 gelu n324": (515, 324, 448, "f8-gelu", "f8"),
    "f8 gate+R 77": (231, 648, 128, "f8-gate+R:77", "f8"),
    "f8 k2240": (96, 648, 2240, "f8", "f8-deep"),
    # persistent blocks: a few more tiles than the grid cap of pipe_grid_x (the CU count, doubled for the four-wave configurations;
    # 256 CUs): 528 tiles of 128 x 128 and of 128 x 160, 288 of 256 x 160, 270 of 256 x 320 and of 256 x 256
    "persist 128": (4224, 2048, 128, "plain", "plain", ("p128", "p128one")),
    "persist 129": (4224, 2560, 128, "plain", "plain", ("p129", "p129one")),
    "persist 160": (4353, 2560, 128, "plain", "plain", ("p160", "p160one")),
    "persist 320": (4353, 4800, 128, "plain", "plain", ("p320", "p320one")),
    "persist 256": (4353, 3840, 128, "plain", "plain", ("p256", "p256one")),
}
COMMON = [n for n, c in CASES.items() if len(c) == 5]


def names_of(sw):
    """the cases a switch set runs: the common matrix (the one-block-per-tile sets: their persistent case alone) + the cases tied to it"""
    tied = [n for n, c in CASES.items() if len(c) == 6 and sw in c[5]]
    return tied if sw.endswith("one") else COMMON + tied


def expected_route(name, sw):
    return ROUTES[sw][CASES[name][4]]


def run_case(name, ed):
    """-> (output [M, N_out], bound check (ratio, rel), guard-band findings)"""
    import torch
    from paddlemix_amd import ops
    from paddlemix_amd.sd3 import quantize_fp8_rows
    from tests import gemm_bounds as GB
    M, N, K, kind = CASES[name][:4]
    rpb = int(kind.split(":")[1]) if ":" in kind else 0
    kind = kind.split(":")[0]
    g = torch.Generator(device="cuda").manual_seed(M * 7 + N * 3 + K)
    lda = K + 64 if kind == "strided" else K
    a = torch.randn(M, lda, device="cuda", generator=g).to(ed)[:, :K]
    if kind.startswith("ln"):   # a row mean several times the row deviation: the fold's two products nearly cancel
        a = (torch.randn(M, K, device="cuda", generator=g) * 0.5 + torch.randn(M, 1, device="cuda", generator=g) * 3.0).to(ed)
    f8 = kind.startswith("f8")
    if f8:
        w, ws = quantize_fp8_rows(torch.randn(N, K, device="cuda", generator=g) / K ** 0.5)
        w_ref = w.view(torch.float8_e4m3fn).float().double() * ws.double()[:, None]   # (the exact product: tests/gemm_bounds.py)
        kind = kind[3:] or "plain"
    else:
        w = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(ed)
        w_ref, ws = w, None
    b = None if kind.endswith("nobias") else torch.randn(N, device="cuda", generator=g)
    nb = (M + rpb - 1) // rpb if rpb else 0
    guard = None
    # bias_acc: a 16-bit launch with a bias may start its accumulators at it (pipelined loops, small tile); never fp8 / LN launches
    bk = dict(bias_acc=b is not None and not f8 and not kind.startswith("ln") and not os.environ.get("MI355X_SD_GEMM_NO_BIAS_ACC"))
    if kind in ("plain", "nobias", "scale", "silu") and not f8:
        sc = 0.7 if kind == "scale" else 1.0
        out = ops.linear(a, w, b, out_scale=sc, silu=kind == "silu")
        bk.update(out_scale=sc, act="silu" if kind == "silu" else None)
    elif kind in ("plain", "nobias", "gelu"):   # linear_ex: tanh-GELU, and every fp8 form
        out = ops.linear_ex(a, w, b, w_scale=ws, gelu_tanh=kind == "gelu")
        bk.update(act="gelu_tanh" if kind == "gelu" else None)
    elif kind == "geglu":
        out = ops.linear(a, w, b, geglu=True)
        bk.update(geglu=True)
    elif kind in ("R", "R-nobias", "Rwide"):
        rbig = torch.randn(M, N + 24, device="cuda", generator=g).to(ed)
        r = rbig[:, 8:8 + N] if kind == "Rwide" else rbig[:, :N].contiguous()
        out = ops.linear(a, w, b, residual=r)
        bk.update(residual=r)
    elif kind == "R32":
        r = torch.randn(M, N, device="cuda", generator=g)
        out = ops.linear(a, w, b, residual=r, out_f32=True)
        bk.update(residual=r)
    elif kind.startswith("rowbias"):
        rb = torch.randn(nb, N, device="cuda", generator=g)
        r, sc, f32 = None, 1.0, kind == "rowbias+R32"
        if kind == "rowbias+R":
            r, sc = torch.randn(M, N, device="cuda", generator=g).to(ed), 0.7
        elif f32:
            r = torch.randn(M, N, device="cuda", generator=g)
        out = ops.linear(a, w, b, rowbias=rb, rows_per_batch=rpb, residual=r, out_scale=sc, out_f32=f32)
        bk.update(rowbias=rb, rows_per_batch=rpb, residual=r, out_scale=sc)
    elif kind == "gate+R":
        gt = torch.randn(nb, N, device="cuda", generator=g)
        r = torch.randn(M, N, device="cuda", generator=g).to(ed)
        out = ops.linear_ex(a, w, b, w_scale=ws, gate=gt, rows_per_batch=rpb, residual=r)
        bk.update(gate=gt, rows_per_batch=rpb, residual=r)
    elif kind == "c-remap":   # batches of 77 rows written behind EXTRA other rows each
        nb = M // 77
        og = KP.Guarded.strided((nb, 77, N), ((77 + EXTRA) * N, N, 1), 0, nb * (77 + EXTRA) * N, 16, dt=ed)
        ops.linear_ex(a, w, b, out=og.buf, c_rows_per_batch=77, c_batch_stride=(77 + EXTRA) * N, M=M)
        out = og.view.reshape(M, N)
        guard = og.counts()[1]
    elif kind == "a-remap":   # A rows of batches of 77 read out of a buffer with EXTRA other rows behind each batch
        nb = M // 77
        abuf = torch.randn(nb * (77 + EXTRA) * K, device="cuda", generator=g).to(ed)
        out = ops.linear_ex(abuf, w, b, a_rows_per_batch=77, a_batch_stride=(77 + EXTRA) * K, M=M)
        a = abuf.view(nb, 77 + EXTRA, K)[:, :77].reshape(M, K)
    elif kind == "strided":
        og = KP.Guarded.block(M, N, 16, above=0, below=40, left=0, right=16, dt=ed)
        out = ops.linear(a, w, b, out=og.view)
        guard = og.counts()[1]
    elif kind.startswith("ln"):
        # the statistics the kernel reads: exact ones rounded to fp32 once (row_stats has its own bound, tests/norm_bounds.py)
        mean, var = a.double().mean(1), a.double().var(1, unbiased=False)
        rstd = torch.rsqrt(var + 1e-5)
        st = torch.stack([rstd, -mean * rstd], 1).float().contiguous()
        wsum = w.float().sum(1).contiguous()
        out = ops.linear_ln(a, st, w, wsum, b, geglu=kind == "ln-geglu")
        bk.update(rowstat=st, wsum=wsum, geglu=kind == "ln-geglu")
    else:
        raise ValueError(kind)
    torch.cuda.synchronize()
    return out, GB.bound_check(out, a, w_ref, bias=b, **bk), guard


def _result(name):
    from paddlemix_amd import _lib
    from tests.gpu_child import sha
    out, (ratio, rel), guard = run_case(name, _lib.elem_dtype())
    return dict(sha=sha(out), ratio=ratio, rel=rel, guard=guard)


if __name__ == "__main__":
    KP.run_cases(COMMON, _result, route_log="MI355X_SD_GEMM_LOG", tag="LINEAR_JSON", names=sys.argv[1:])
