"""Child of tests/test_gpu_attention.py: the case matrix of the attention kernels (csrc/attention.hip, every form launch_dp launches)
on the inputs of tests/attn_cases.py. Every case is held to the elementwise float64 bound of tests/attn_bounds.py over its WHOLE
output (the reference runs on the device). The output is a view inside a larger buffer of canary NaNs (row padding, batch padding,
a 16-byte-aligned or an only 8-byte-aligned base), K and V views inside NaN buffers (rows behind Skv, columns behind the last head).
With MI355X_SD_ATTN_LOG set (debug build) each case also reports the kernel family launch_attention logged for it. Prints one JSON
line: per case worst err / bound, rel-L2, unwritten / overwritten element counts, bit-equality with v (Skv = 1), route.

  python tests/attn_child.py [case ...]     (no names: every case)
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from paddlemix_amd import _lib, ops  # noqa: E402
from tests import attn_bounds as AB  # noqa: E402
from tests import attn_cases as AC  # noqa: E402
from tests import kernel_pieces as KP  # noqa: E402

CASES = {}        # name: (spec, family the route log must show, aligned O)


def _add(name, fam, B, H, Sq, Skv, D, kind, bias=None, log2=False, accum=None, aligned=True, ninf=False):
    CASES[name] = (dict(B=B, H=H, Sq=Sq, Skv=Skv, D=D, kind=kind, bias=bias, log2=log2, accum=accum, ninf=ninf), fam, aligned)


# short key sequences at D = 64: the single-pass kernel, NSB = ceil(Skv / 32) blocks of 32 keys
for i, (Skv, Sq) in enumerate(((1, 1), (32, 77), (33, 129), (64, 200), (65, 300), (96, 129), (97, 257), (128, 333))):
    nsb = (Skv + 31) // 32
    for log2 in (False, True):
        kind = "S3" if Skv == 1 else ("S1", "S2", "S4")[(i + log2) % 3]
        _add(f"short Skv{Skv} Sq{Sq}{' log2' if log2 else ''} {kind}", f"short/{nsb}" + ("+log2" if log2 else ""), 2, 3, Sq, Skv, 64,
             kind, log2=log2)
# two query tiles per block: Skv <= 128, >= 1024 query tiles, the short kernel declining (D < 64, accum, unaligned O)
for kind in ("S1", "S2", "S4"):
    _add(f"qt2 D40 1024 tiles {kind}", "flash64/qt2", 8, 8, 2048, 77, 40, kind)
_add("qt2 D40 odd tiles ragged Sq S2", "flash64/qt2", 8, 16, 1100, 128, 40, "S2")
_add("qt2 D40 Skv65 S1", "flash64/qt2", 8, 16, 1100, 65, 40, "S1")
_add("qt2 D40 Skv1 S3", "flash64/qt2", 8, 8, 2048, 1, 40, "S3")
_add("qt2 log2 D64 unaligned S2", "flash64/qt2+log2", 8, 8, 2048, 77, 64, "S2", log2=True, aligned=False)
_add("qt2 log2 D64 unaligned S4", "flash64/qt2+log2", 8, 16, 1100, 97, 64, "S4", log2=True, aligned=False)
_add("qt2 D64 accum S4", "flash64/qt2", 8, 8, 2048, 77, 64, "S4", accum=0.6)
_add("1023 query tiles D40 S2", "flash64+lazy", 3, 11, 3968, 77, 40, "S2")
# the 16x16x32 kernel: D = 64, 16-byte O rows, no mask, Skv > 128
for i, Skv in enumerate((129, 192, 4096, 4250)):
    Sq = 257 if Skv < 4096 else Skv
    for log2 in (False, True):
        kind = ("S1", "S2", "S4", "S2g")[(i + 2 * log2) % 4]
        _add(f"m16 Skv{Skv}{' log2' if log2 else ''} {kind}", "m16" + ("+log2" if log2 else ""), 1, 2, Sq, Skv, 64, kind, log2=log2)
# the d <= 64 flash kernel: lazy (and wide where D % 16 == 0)
for i, D in enumerate((8, 16, 32, 40, 48, 56)):
    fam = "flash64+lazy" + ("+wide" if D % 16 == 0 else "")
    for kind in (("S1", "S2", "S4", "S2g")[i % 4], ("S2", "S4", "S2g", "S1")[i % 4]):
        _add(f"flash64 D{D} {kind}", fam, 2, 3, 200, 193, D, kind)
# (the log2 form takes D = 64 only; with 16-byte O rows the 16x16x32 kernel takes it, so its wide flash form runs where that kernel is
# switched off: MI355X_SD_ATTN_NO_M16, the A/B switch of the debug build -- the cases named "nom16", run in a child of their own)
_add("nom16 D64 log2 S2g", "flash64+log2+wide", 2, 3, 200, 300, 64, "S2g", log2=True)
_add("nom16 D64 log2 S1", "flash64+log2+wide", 2, 3, 200, 130, 64, "S1", log2=True)
_add("nom16 D64 log2 S4", "flash64+log2+wide", 1, 2, 257, 4250, 64, "S4", log2=True)
_add("nom16 D64 S2", "flash64+lazy+wide", 2, 3, 200, 193, 64, "S2")
_add("flash64 D64 unaligned S2g", "flash64+lazy", 2, 3, 200, 300, 64, "S2g", aligned=False)
_add("flash64 D64 unaligned S1", "flash64+lazy", 2, 3, 129, 65, 64, "S1", aligned=False)
_add("flash64 D64 unaligned log2 S4", "flash64+log2", 2, 3, 200, 300, 64, "S4", log2=True, aligned=False)
_add("flash64 D64 unaligned log2 S2", "flash64+log2", 2, 3, 200, 193, 64, "S2", log2=True, aligned=False)
_add("flash64 D64 accum S2", "flash64+lazy", 2, 3, 200, 193, 64, "S2", accum=0.6)
_add("flash64 D64 accum S1", "flash64+lazy", 2, 3, 200, 77, 64, "S1", accum=-0.35)
_add("flash64 D40 accum S4", "flash64+lazy", 2, 3, 200, 77, 40, "S4", accum=0.6)
_add("flash64 D40 Skv1 S3", "flash64+lazy", 2, 3, 200, 1, 40, "S3")
_add("flash64 D64 unaligned Skv1 S3", "flash64+lazy", 2, 3, 200, 1, 64, "S3", aligned=False)
# masks on the d <= 64 flash kernel: every bias layout
_add("flash64 bias bhqk S2b", "flash64+bias", 2, 3, 200, 193, 64, "S2b", bias="bhqk")
_add("flash64 bias 1hqk S2b", "flash64+bias", 2, 3, 200, 130, 40, "S2b", bias="1hqk")
_add("flash64 bias b11k S2b", "flash64+bias", 2, 3, 200, 77, 64, "S2b", bias="b11k")
_add("flash64 bias bhqk S2", "flash64+bias", 2, 3, 200, 256, 64, "S2", bias="bhqk")
_add("flash64 bias b11k S4", "flash64+bias", 2, 3, 200, 300, 64, "S4", bias="b11k")
_add("flash64 keep S1", "flash64+bias", 2, 3, 200, 77, 64, "S1", bias="keep")
_add("flash64 unet log2 mask S1", "flash64+bias", 2, 3, 200, 77, 64, "S1", bias="unet")
_add("flash64 unet log2 mask S4", "flash64+bias", 2, 3, 200, 300, 64, "S4", bias="unet")
_add("flash64 bias accum S4", "flash64+bias", 2, 3, 200, 130, 64, "S4", bias="b11k", accum=0.6)
_add("flash64 bias Skv1 S3", "flash64+bias", 2, 3, 200, 1, 64, "S3", bias="bhqk")
_add("flash64 -inf rows S4", "flash64+bias", 2, 3, 200, 193, 64, "S4", bias="bhqk", ninf=True)
# head dims padded to DP = 96 (two LDS buffers) and DP = 160 (one buffer, reloaded between barriers)
for i, D in enumerate((72, 80, 88, 96)):
    for j, Skv in enumerate((77, 256, 1000)):
        kind = ("S1", "S2", "S4", "S2g")[(i + j) % 4]
        _add(f"flash96 D{D} Skv{Skv} {kind}", "flash96", 2, 3, 200 if Skv < 1000 else 130, Skv, D, kind, aligned=(i + j) % 2 == 0)
_add("flash96 D72 bias bhqk S2b", "flash96+bias", 2, 3, 200, 256, 72, "S2b", bias="bhqk")
_add("flash96 D80 bias 1hqk S2b", "flash96+bias", 2, 3, 200, 77, 80, "S2b", bias="1hqk")
_add("flash96 D88 bias b11k S2b", "flash96+bias", 2, 3, 130, 1000, 88, "S2b", bias="b11k")
_add("flash96 D96 keep S1", "flash96+bias", 2, 3, 200, 256, 96, "S1", bias="keep")
_add("flash96 D72 unet S4", "flash96+bias", 2, 3, 200, 77, 72, "S4", bias="unet")
_add("flash96 D72 accum S2", "flash96", 2, 3, 200, 256, 72, "S2", accum=0.6)
_add("flash96 D80 Skv1 S3", "flash96", 2, 3, 200, 1, 80, "S3")
_add("flash96 -inf rows S4", "flash96+bias", 2, 3, 200, 256, 72, "S4", bias="bhqk", ninf=True)
for i, D in enumerate((104, 128, 160)):
    for j, Skv in enumerate((64, 65, 257, 1024)):
        kind = ("S1", "S2", "S4", "S2g")[(i + j) % 4]
        _add(f"flash160 D{D} Skv{Skv} {kind}", "flash160", 2, 3, 200 if Skv < 1024 else 130, Skv, D, kind, aligned=(i + j) % 2 == 1)
_add("flash160 D104 bias bhqk S2b", "flash160+bias", 2, 3, 200, 257, 104, "S2b", bias="bhqk")
_add("flash160 D128 bias 1hqk S2b", "flash160+bias", 2, 3, 200, 65, 128, "S2b", bias="1hqk")
_add("flash160 D160 keep S1", "flash160+bias", 2, 3, 200, 257, 160, "S1", bias="keep")
_add("flash160 D160 accum S2", "flash160", 2, 3, 200, 257, 160, "S2", accum=0.6)
_add("flash160 D128 Skv1 S3", "flash160", 2, 3, 200, 1, 128, "S3")


def _geom(B, S, H, D, row_pad, extra_rows, off):
    """(shape, strides, off, n) of a [B, S, H, D] view in a flat buffer: rows H*D + row_pad and batches S + extra_rows rows apart, from `off`, 64 behind"""
    ts = H * D + row_pad
    bs = (S + extra_rows) * ts
    return (B, S, H, D), (bs, ts, D, 1), off, off + B * bs + 64


def run_case(name):
    spec, _, aligned = CASES[name]
    ed = _lib.elem_dtype()
    c = AC.make(spec, ed, device="cuda", seed=sum(map(ord, name)))
    if spec["ninf"]:   # rows whose keys are all masked with -inf (0 by convention), one row masked in its first tile only
        c["bias"][0, 1, 3] = -math.inf
        c["bias"][1, 2, 5, :64] = -math.inf
    B, Sq, H, D = c["q"].shape
    Skv = c["k"].shape[1]
    # K, V: NaN rows behind Skv (40 of them), NaN columns behind the last head (16)
    kv = [KP.nan_embed(t, *_geom(B, Skv, H, D, 16, 40, 0)[1:])[0] for t in (c["k"], c["v"])]
    # O: 16-byte-aligned base and rows (the 16-byte store forms), or an 8-byte-aligned base and rows (the 8-byte forms)
    og = KP.Guarded.strided(*_geom(B, Sq, H, D, 8 if aligned else 4, 3, 0 if aligned else 4), 16, dt=ed)
    out = og.view
    if c["accum"] is not None:
        out.copy_(c["old"])
    scale = None if c["log2"] else c["scale"]
    ops.sdpa(c["q"], kv[0], kv[1], bias=c["bias"], scale=scale, out=out, accum=c["accum"], log2=c["log2"])
    torch.cuda.synchronize()
    unwritten, overwritten = og.counts()
    ratio, rel = AB.bound_check(out, c["q"], c["k"], c["v"], scale=c["scale"], bias=c["bias"], log2=c["log2"], accum=c["accum"],
                                old=c["old"], exact_p=c["exact_p"])
    same_v = None
    if spec["kind"] == "S3" and c["accum"] is None:
        same_v = bool(torch.equal(out.view(torch.int16), c["v"].expand(B, Sq, H, D).view(torch.int16)))
    zero_rows = None
    if spec["ninf"]:
        zero_rows = bool((out[0, 3, 1] == 0).all().item())
    return dict(ratio=ratio, rel=rel, unwritten=unwritten, overwritten=overwritten, same_v=same_v, zero_rows=zero_rows)


if __name__ == "__main__":
    KP.run_cases(CASES, run_case, route_log="MI355X_SD_ATTN_LOG", tag="ATTN_JSON", names=sys.argv[1:])
