"""Child of tests/test_gpu_convs.py: the convolution case matrix of tests/conv_cases.py under the MI355X_SD_* switches of its
environment (read once per process). Selector cases are compared exactly, random cases are held to the elementwise float64 bound of
tests/conv_bounds.py over the WHOLE output; inputs sit in NaN buffers, outputs in canary buffers; with MI355X_SD_GEMM_LOG set (debug
build) each case also reports the kernel family launch_gemm logged for it. One launch per case. Prints one JSON line.

  python tests/conv_child.py gemm [case ...]     mi355x_sd_conv3x3 (no names: every case)
  python tests/conv_child.py direct              conv_in3x3, conv_out3x3, conv1x1_nchw (csrc/misc.hip)
  python tests/conv_child.py wide                one stride-2 conv whose source spans 6 GiB (32-bit offsets cannot address it)
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from paddlemix_amd import _lib, ops  # noqa: E402
from tests import conv_bounds as CB  # noqa: E402
from tests import conv_cases as CC  # noqa: E402
from tests import kernel_pieces as KP  # noqa: E402
from tests.gpu_child import Routes, emit, sha  # noqa: E402


def run_gemm_case(name):
    ed = _lib.elem_dtype()
    case = CC.CASES[name]
    d = CC.build(name, case, ed, "cuda")
    s, up, br = CC.GEOMS[case.geom]
    og = CC.alloc_out(d["M"], case.Cout, torch.float32 if d["out_f32"] else ed, "cuda")
    out = og.view
    ops.conv3x3(d["x"], d["w_dev"], d["bias"], stride=s, upsample=up, rowbias=d["rowbias"], residual=d["residual"], out=out,
                out_scale=d["out_scale"], pad_br=br, kb64=case.kb64, silu=d["silu"], out_f32=d["out_f32"])
    torch.cuda.synchronize()
    res = CC.judge(case, d, out)
    res.update(guard=og.counts()[1], sha=sha(out), M=d["M"])
    return res


# ---- the three direct kernels ---------------------------------------------------------------------------------------------------
MARGIN = 4096   # elements of NaN in front of and behind a dense fp32 input, of canary around a dense fp32 output


def nan_margins(x):
    """a dense fp32 tensor -> the same values in the middle of a NaN-filled allocation (a read outside the tensor poisons the result)"""
    return KP.nan_embed(x, x.contiguous().stride(), MARGIN, x.numel() + 2 * MARGIN)


def canary_nchw(shape):
    """a dense fp32 NCHW output in the middle of a canary-filled allocation (KP.Guarded: .view, .counts()[1] the disturbed margin)"""
    return KP.Guarded.strided(shape, torch.empty(shape, device="meta").stride(), MARGIN, math.prod(shape) + 2 * MARGIN, 32)


def _exact_or_bound(out, ref, e, exact):
    if exact:
        bad = int((out.double() != ref).sum().item())
        return dict(ratio=0.0 if bad == 0 else float("inf"), rel=0.0, mismatch=bad)
    ratio, rel = CB.check(out, ref, e)
    return dict(ratio=ratio, rel=rel, mismatch=None)


def conv_in_case(ed, kind, Cin, Cout, B, H, W, scale, f32, seed):
    """w [9 Cin][Cout]; selectors: one-hot rows k(n) (coded x) or the tap powers (x = 1); W is no multiple of the 4 pixels a thread owns"""
    lib = _lib.load()
    g = torch.Generator().manual_seed(seed)
    K = 9 * Cin
    bias = None
    if kind == "coded":
        x = CC.coded_x(B, H, W, Cin, "cuda").permute(0, 3, 1, 2).contiguous()
        w = torch.zeros(K, Cout)
        w[CC.selector_k(Cout, K, seed), torch.arange(Cout)] = 1.0
    elif kind == "mask":
        x = torch.ones(B, Cin, H, W, device="cuda")
        w = CC.mask_w(Cout, Cin).t().contiguous()
    else:
        x = torch.randn(B, Cin, H, W, generator=g).cuda()
        w = CC.exact16(torch.randn(K, Cout, generator=g) / math.sqrt(K))
        bias = torch.randn(Cout, generator=g).cuda()
    w = w.cuda().to(ed)
    x, x_full = nan_margins(x)
    sc = torch.tensor([scale], dtype=torch.float32, device="cuda") if scale is not None else None
    M = B * H * W
    og = CC.alloc_out(M, Cout, torch.float32 if f32 else ed, "cuda")
    out = og.view
    _lib.check(lib.mi355x_sd_conv_in3x3_ex(x.data_ptr(), sc.data_ptr() if sc is not None else None, w.data_ptr(),
                                           bias.data_ptr() if bias is not None else None, out.data_ptr(), B, Cin, H, W, Cout,
                                           out.stride(0), int(f32), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ref, e = CB.conv_in3x3_reference(x, w, bias, sc, ed)
    r = _exact_or_bound(out, ref, e, kind != "random")
    r["guard"] = og.counts()[1]
    return r


def conv_out_case(ed, kind, Cin, Cout, B, H, W, seed, tap0=0):
    """x a strided view in a NaN buffer; w [Cout][9][Cin]; the coded selector takes taps tap0 .. tap0 + Cout - 1 (the caller walks tap0)"""
    g = torch.Generator().manual_seed(seed)
    K = 9 * Cin
    bias = None
    if kind == "coded":
        x = CC.coded_x(B, H, W, Cin, "cuda")
        w = torch.zeros(Cout, 9, Cin)
        for n in range(Cout):
            w[n, (tap0 + n) % 9, (seed * 7 + 9 * n + 67 * tap0) % Cin] = 1.0
        w = w.reshape(Cout, K)
    elif kind == "mask":
        x = torch.ones(B, H, W, Cin, device="cuda")
        w = CC.mask_w(Cout, Cin)
    else:
        x = CC.exact16(torch.randn(B, H, W, Cin, generator=g)).cuda()
        w = CC.exact16(torch.randn(Cout, K, generator=g) / math.sqrt(K))
        bias = torch.randn(Cout, generator=g).cuda()
    w = w.cuda().to(ed)
    view, full, first = CC.nan_embedded(x.to(ed))
    rows = full.as_strided((B * H * W, Cin), (Cin + CC.X_GAP, 1), first)
    og = canary_nchw((B, Cout, H, W))
    out = og.view
    _lib.check(_lib.load().mi355x_sd_conv_out3x3(rows.data_ptr(), rows.stride(0), w.data_ptr(), bias.data_ptr() if bias is not None else None,
                                                 out.data_ptr(), B, Cin, H, W, Cout, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ref, e = CB.conv_out3x3_reference(view, w, bias)
    r = _exact_or_bound(out, ref, e, kind != "random")
    r["guard"] = og.counts()[1]
    return r


def conv1x1_case(ed, kind, Cin, Cout, B, H, W, scale, seed):
    g = torch.Generator().manual_seed(seed)
    bias = None
    if kind == "coded":   # (0.5 x an integer <= 126: still exact in 8 significand bits)
        x = CC.coded_x(B, H, W, Cin, "cuda").permute(0, 3, 1, 2).contiguous()
        w = torch.zeros(Cout, Cin)
        w[torch.arange(Cout), (5 * torch.arange(Cout) + seed) % Cin] = 1.0
    else:
        x = torch.randn(B, Cin, H, W, generator=g).cuda()
        w = CC.exact16(torch.randn(Cout, Cin, generator=g) / math.sqrt(Cin))
        bias = torch.randn(Cout, generator=g).cuda()
    w = w.cuda().to(ed)
    x, x_full = nan_margins(x)
    og = canary_nchw((B, Cout, H, W))
    out = og.view
    _lib.check(_lib.load().mi355x_sd_conv1x1_nchw(x.data_ptr(), float(scale), w.data_ptr(), bias.data_ptr() if bias is not None else None,
                                                  out.data_ptr(), B, Cin, Cout, H * W, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ref, e = CB.conv1x1_nchw_reference(x, w, bias, scale, ed)
    r = _exact_or_bound(out, ref, e, kind != "random")
    r["guard"] = og.counts()[1]
    return r


def main_direct():
    ed = _lib.elem_dtype()
    res = {}
    n = 0
    for Cin in (4, 8):   # the unrolled (Cin = 4) and the rolled form
        for kind in ("coded", "mask", "random"):
            for scale in (None, 0.5 if kind != "random" else 0.18215):
                for f32 in (False, True):
                    n += 1
                    res[f"conv_in {kind} cin{Cin} scale={scale} f32={f32}"] = conv_in_case(ed, kind, Cin, 40, 2, 5, 7, scale, f32, n)
    res["conv_in random cin4 320 out 2x33x31"] = conv_in_case(ed, "random", 4, 320, 2, 33, 31, 0.18215, False, 99)
    for Cin in (64, 320):
        for t0 in range(9):   # (4 selected elements per launch: every tap four times, at channels spread over Cin)
            res[f"conv_out coded cin{Cin} taps {t0}.."] = conv_out_case(ed, "coded", Cin, 4, 2, 5, 7, Cin + t0, tap0=t0)
        res[f"conv_out mask cin{Cin}"] = conv_out_case(ed, "mask", Cin, 2, 2, 5, 7, 3)
        res[f"conv_out random cin{Cin}"] = conv_out_case(ed, "random", Cin, 4, 2, 9, 7, 4)
    res["conv_out random cin128 cout3 1x1 image"] = conv_out_case(ed, "random", 128, 3, 2, 1, 1, 5)
    res["conv1x1 coded 4->8"] = conv1x1_case(ed, "coded", 4, 8, 2, 5, 7, 0.5, 1)
    res["conv1x1 coded 16->16"] = conv1x1_case(ed, "coded", 16, 16, 2, 3, 5, 1.0, 2)
    res["conv1x1 random 4->4"] = conv1x1_case(ed, "random", 4, 4, 2, 9, 7, 1 / 0.18215, 3)
    res["conv1x1 random 16->16"] = conv1x1_case(ed, "random", 16, 16, 3, 5, 3, 1 / 0.13025, 4)
    return res


def main_wide():
    """3 x 1024 x 1024 pixels, pixel stride 1024 (a 64-channel slice), stride 2: the source spans 6 GiB while M * lda stays below 2^30
    elements -- the picker's 256 x 256 choice. The last image (behind the 4-GiB line) against the float64 reference on the device."""
    ed = _lib.elem_dtype()
    B, H, W, Cin, Cout, ldx = 3, 1024, 1024, 64, 256, 1024
    g = torch.Generator(device="cuda").manual_seed(11)
    full = torch.empty(B, H, W, ldx, device="cuda", dtype=ed)
    for b in range(B):
        full[b] = torch.randn(H, W, ldx, device="cuda", generator=g).to(ed)
    x = full[..., 64:64 + Cin]
    w = (torch.randn(Cout, 9 * Cin, device="cuda", generator=g) / 24).to(ed)
    bias = torch.randn(Cout, device="cuda", generator=g)
    routes = Routes("MI355X_SD_GEMM_LOG")
    routes.take()
    out = ops.conv3x3(x, CB.to_kb64(w), bias, stride=2, kb64=True)
    torch.cuda.synchronize()
    route = routes.take()
    rows = out.shape[0] // B
    ref, e = CB.conv3x3_reference(x[B - 1:], w, stride=2, bias=bias)
    ratio, rel = CB.check(out[(B - 1) * rows:], ref, e)
    ref0, e0 = CB.conv3x3_reference(x[:1, :64], w, stride=2, bias=bias)   # and the first rows of the first image
    r0, _ = CB.check(out[:31 * 512], ref0[:31 * 512], e0[:31 * 512])
    return {"wide": dict(ratio=max(ratio, r0), rel=rel, route=route, src_bytes=full.numel() * 2)}


if __name__ == "__main__":
    if sys.argv[1] == "gemm":
        KP.run_cases(CC.CASES, run_gemm_case, route_log="MI355X_SD_GEMM_LOG", tag="CONV_JSON", names=sys.argv[2:])
    else:
        ops.init(0)
        emit("CONV_JSON", main_direct() if sys.argv[1] == "direct" else main_wide())
