#!/usr/bin/env python
"""Per-launch time of mi355x_sd_freeu at the six SDXL concat shapes (B = 8), next to mi355x_sd_scale_shift_act on the same buffers
in the same process -- a streaming kernel of the same layout. HIP events around ITERS back-to-back calls after WARM warm-up calls,
median of REPS. The concat buffer is 42 MB (32 x 32, 1280/1280) to 126 MB (64 x 64, 1280/640); FreeU works in it, scale_shift_act
(whose x and y are declared not to alias) also writes a second buffer of the same size, 84 - 252 MB together. Next to the 256 MiB
Infinity Cache that leaves FreeU's footprint cache-resident at every shape and scale_shift_act's at all but the largest, where it
is at the cache's edge: the rates are repeated-call rates, comparable with each other and not with the HBM roof, and the footprints
differ in FreeU's favour. Bytes: FreeU reads the skip columns twice (statistics, apply), writes them once, and reads and writes the
scaled backbone half; scale_shift_act reads and writes every column once.

    python scripts/freeu_bench.py > profiles/<name>.txt"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from paddlemix_amd import _lib   # noqa: E402

SHAPES = [(32, 1280, 1280), (32, 1280, 1280), (32, 1280, 640), (64, 1280, 640), (64, 640, 640), (64, 640, 320)]   # (H = W, Cx, Cs)
B, WARM, ITERS, REPS = 8, 5, 20, 5


def timed(fn):
    for _ in range(WARM):
        fn()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / ITERS)
    return statistics.median(out), min(out), max(out)


def main():
    lib = _lib.load()
    _lib.check(lib.mi355x_sd_init(0))
    st = torch.cuda.current_stream().cuda_stream
    print(f"# {_lib.ELEM_NAME} elements, B = {B}; us per call: median (min .. max) of {REPS} x {ITERS} calls")
    print("# shape HxW Cx/Cs | freeu us | freeu GB moved | freeu GB/s | scale_shift_act us | GB | GB/s | freeu rate / ssa rate")
    for hw, cx, cs in SHAPES:
        C, rows = cx + cs, B * hw * hw
        cat = torch.randn(rows, C, device="cuda").to(_lib.elem_dtype())
        ws = torch.empty(lib.mi355x_sd_freeu_workspace_floats(B, hw, hw, cs), dtype=torch.float32, device="cuda")
        ss = torch.ones(B * 2 * C, dtype=torch.float32, device="cuda")
        y = torch.empty_like(cat)
        fu = lambda: _lib.check(lib.mi355x_sd_freeu(cat.data_ptr(), C, B, hw, hw, cx, cs, 1.0, 1.0, 0, ws.data_ptr(), st))  # noqa: E731
        sa = lambda: _lib.check(lib.mi355x_sd_scale_shift_act(cat.data_ptr(), B, hw * hw, C, C, ss.data_ptr(), 0, y.data_ptr(), C, st))  # noqa: E731
        tf, ts = timed(fu), timed(sa)
        bf = 2.0 * rows * (3 * cs + 2 * (cx // 2))
        bs = 2.0 * rows * 2 * C
        rf, rs = bf / tf[0] * 1e-3, bs / ts[0] * 1e-3
        print(f"{hw}x{hw} {cx}/{cs} | {tf[0]:.1f} ({tf[1]:.1f} .. {tf[2]:.1f}) | {bf * 1e-9:.4f} | {rf:.0f} | {ts[0]:.1f} ({ts[1]:.1f} .. {ts[2]:.1f}) | "
              f"{bs * 1e-9:.4f} | {rs:.0f} | {rf / rs:.2f}")


if __name__ == "__main__":
    main()
