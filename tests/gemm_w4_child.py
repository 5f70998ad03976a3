"""Child of tests/test_gpu_gemm_w4.py: the case matrix of the four-wave GEMM tile (csrc/gemm_w4.hip, 256 x 256 and 256 x 160 forms)
under the MI355X_SD_* switches of its environment (read once per process). Every case is held to the elementwise float64 bound of
tests/gemm_bounds.py over its WHOLE output; with MI355X_SD_GEMM_LOG set (debug build) each case also reports the kernel family
launch_gemm logged for it. Prints one JSON line: per case sha256 of the output, worst err / bound, rel-L2, route.

  python tests/gemm_w4_child.py [case ...]     (no names: every case)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from paddlemix_amd import _lib, ops  # noqa: E402
from paddlemix_amd.sd3 import dequantize_fp8_rows, quantize_fp8_rows  # noqa: E402
from tests import gemm_bounds as GB  # noqa: E402
from tests import kernel_pieces as KP  # noqa: E402
from tests.gpu_child import sha  # noqa: E402


# name: (M, N, K, kind, picker) -- picker: the launch is one the picker gives the four-wave 256 x 256 tile (M >= 2048, N >= 1536,
# >= 192 tiles of 256 x 256). kind: plain | nobias | scale | silu | gelu (tanh, linear_ex) | geglu | gate+R:<rows per batch> |
# R (residual, no gate) | c-remap | a-remap | ws-plain | ws-gelu | ws-gate+R | strided (lda = K + 64, out= view with ldc = N + 16
# inside a canary buffer with 256 spare rows)
CASES = {
    # K: three K-tiles (the main loop runs zero times), four, five, 20, 96
    "k192": (8192, 1536, 192, "plain", True),
    "k256": (8192, 1536, 256, "plain", True),
    "k320": (8192, 1536, 320, "plain", True),
    "qkv k1280": (8192, 3840, 1280, "plain", True),
    "k6144": (8192, 1536, 6144, "plain", True),
    # rounds of persistent blocks
    "m300 (fewer tiles than CUs)": (300, 1536, 1280, "plain", False),
    "256 tiles": (4096, 4096, 640, "plain", True),
    "257 tiles": (65792, 256, 256, "plain", False),
    "several rounds": (33000, 1536, 1536, "plain", True),
    "186 tiles (below the picker)": (7936, 1536, 640, "plain", False),
    "192 tiles (the picker's threshold)": (8192, 1536, 640, "nobias", True),
    # ragged edges
    "m%256=1": (8193, 1536, 640, "plain", True),
    "m%256=255": (8191, 1536, 640, "plain", True),
    "n%16=8": (8192, 1560, 640, "plain", True),
    "n%256=8": (8192, 2312, 640, "plain", True),
    "geglu n%256=32": (8192, 3104, 640, "geglu", True),
    # epilogues
    "nobias": (8192, 3840, 1280, "nobias", True),
    "out_scale": (8192, 1536, 640, "scale", True),
    "silu": (8192, 1536, 640, "silu", True),
    "gelu_tanh": (8192, 6144, 1536, "gelu", True),
    "ff1 geglu": (8192, 10240, 1280, "geglu", True),
    # EX: gate + residual, residual alone (no carried prologue), row remaps
    "ex gate+R rpb256": (8192, 1536, 1536, "gate+R:256", True),
    "ex gate+R rpb2048": (8192, 1536, 1536, "gate+R:2048", True),
    "ex gate+R 16384x1536x6144": (16384, 1536, 6144, "gate+R:4096", True),
    "ex R": (8192, 1536, 1280, "R", True),
    "ex c-remap rpb256": (8192, 1536, 1536, "c-remap", True),
    "ex a-remap rpb256": (8192, 1536, 1536, "a-remap", True),
    # WS: a widened e4m3 matrix
    "ws plain": (8192, 1536, 1536, "ws-plain", True),
    "ws gelu_tanh": (8192, 6144, 1536, "ws-gelu", True),
    "ws gate+R": (8192, 1536, 1536, "ws-gate+R", True),
    # strides and guard bands
    "strided": (8192, 1536, 640, "strided", True),
}
EXTRA = 154   # rows of other data between the batches of a remapped operand


def run_case(name, ed):
    """-> (output [M, N_out], bound check (ratio, rel), guard-band findings)"""
    M, N, K, kind, _ = CASES[name]
    g = torch.Generator(device="cuda").manual_seed(M * 7 + N * 3 + K)
    lda = K + 64 if kind == "strided" else K
    a_full = torch.randn(M, lda, device="cuda", generator=g).to(ed)
    a = a_full[:, :K]
    if kind.startswith("ws"):
        w8, ws = quantize_fp8_rows(torch.randn(N, K, device="cuda", generator=g) / K ** 0.5)
        w_ref = dequantize_fp8_rows(w8, ws)
    else:
        w = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(ed)
        w_ref = w
    b = None if kind == "nobias" else torch.randn(N, device="cuda", generator=g)
    bk = {}
    guard = None
    if kind in ("plain", "nobias", "scale", "silu"):
        sc = 0.7 if kind == "scale" else 1.0
        out = ops.linear(a, w, b, out_scale=sc, silu=kind == "silu")
        bk = dict(out_scale=sc, act="silu" if kind == "silu" else None)
    elif kind == "geglu":
        out = ops.linear(a, w, b, geglu=True)
        bk = dict(geglu=True)
    elif kind == "gelu":
        out = ops.linear_ex(a, w, b, gelu_tanh=True)
        bk = dict(act="gelu_tanh")
    elif kind.startswith("gate+R") or kind == "ws-gate+R":
        rpb = int(kind.split(":")[1]) if ":" in kind else 2048
        gt = torch.randn(M // rpb, N, device="cuda", generator=g)
        r = torch.randn(M, N, device="cuda", generator=g).to(ed)
        if kind.startswith("ws"):
            out = ops.linear_ex(a, w8, b, w_scale=ws, gate=gt, rows_per_batch=rpb, residual=r)
        else:
            out = ops.linear_ex(a, w, b, gate=gt, rows_per_batch=rpb, residual=r)
        bk = dict(gate=gt, rows_per_batch=rpb, residual=r)
    elif kind == "R":
        r = torch.randn(M, N, device="cuda", generator=g).to(ed)
        out = ops.linear(a, w, b, residual=r, out_scale=0.5)
        bk = dict(residual=r, out_scale=0.5)
    elif kind == "c-remap":   # batches of 256 rows written behind EXTRA other rows each
        nb = M // 256
        og = KP.Guarded.strided((nb, 256, N), ((256 + EXTRA) * N, N, 1), 0, nb * (256 + EXTRA) * N, 16, dt=ed)
        ops.linear_ex(a, w, b, out=og.buf, c_rows_per_batch=256, c_batch_stride=(256 + EXTRA) * N, M=M)
        out = og.view.reshape(M, N)
        guard = og.counts()[1]
    elif kind == "a-remap":   # A rows of batches of 256 read out of a buffer with EXTRA other rows behind each batch
        nb = M // 256
        abuf = torch.randn(nb * (256 + EXTRA) * K, device="cuda", generator=g).to(ed)
        out = ops.linear_ex(abuf, w, b, a_rows_per_batch=256, a_batch_stride=(256 + EXTRA) * K, M=M)
        a = abuf.view(nb, 256 + EXTRA, K)[:, :256].reshape(M, K)
    elif kind == "ws-plain":
        out = ops.linear_ex(a, w8, b, w_scale=ws)
    elif kind == "ws-gelu":
        out = ops.linear_ex(a, w8, b, w_scale=ws, gelu_tanh=True)
        bk = dict(act="gelu_tanh")
    elif kind == "strided":
        og = KP.Guarded.block(M, N, 16, above=0, below=256, left=0, right=16, dt=ed)
        out = ops.linear(a, w, b, out=og.view)
        guard = og.counts()[1]
    else:
        raise ValueError(kind)
    torch.cuda.synchronize()
    return out, GB.bound_check(out, a, w_ref, bias=b, **bk), guard


def _result(name):
    out, (ratio, rel), guard = run_case(name, _lib.elem_dtype())
    return dict(sha=sha(out), ratio=ratio, rel=rel, guard=guard)


if __name__ == "__main__":
    KP.run_cases(CASES, _result, route_log="MI355X_SD_GEMM_LOG", tag="W4_JSON", names=sys.argv[1:])
