"""CPU: the guarded output and the NaN embedding of tests/kernel_pieces.py on device="cpu" buffers. Each constructor: a write inside
the view alone counts (0, 0), one unwritten inside element (1, 0), one write in a row gap, in a row behind the end, before the base
offset (0, 1) each. And the geometry of two existing cases per family -- offset, strides and buffer length as the helpers these
pieces replaced produced them, stated as literals -- with the arguments the family's child passes."""
import pytest
import torch

from tests import conv_cases as CC
from tests import kernel_pieces as KP
from tests.gemm_f8_bounds import row_offsets

HF = torch.float16


def _fill(g, value=1.0):
    """a kernel that writes exactly its output"""
    if hasattr(g, "idx"):
        g.buf[g.idx] = value
    else:
        g.view.fill_(value)
    return g


# name: (constructor, element offsets outside the view that a stray store could hit)
def _guards():
    attn = KP.Guarded.strided((2, 5, 3, 8), (8 * 28, 28, 8, 1), 4, 4 + 2 * 8 * 28 + 64, 16, dt=HF, device="cpu")   # off 4, 3 extra rows
    rows = KP.Guarded.rows((4, 24), 32, 16, extra_rows=3, tail=64, dt=HF, device="cpu")
    rows3 = KP.Guarded.rows((2, 3, 8), 12, 32, extra_rows=3, tail=64, device="cpu")
    rows8 = KP.Guarded.rows((5, 16), 24, 8, extra_rows=3, tail=64, device="cpu")
    block = KP.Guarded.block(6, 10, 16, above=2, below=3, left=8, right=8, dt=HF, device="cpu")
    idx = 40 + row_offsets(6, 16, 3, 5 * 16)[:, None] + torch.arange(12)   # batches of 3 rows inside 5, from row 2.5 on
    at = KP.Guarded.at(idx, 13 * 16 + 64, 16, base=40, dt=HF, device="cpu")
    at8 = KP.Guarded.at(row_offsets(4, 16)[:, None] + torch.arange(12), 7 * 16 + 64, 8, base=0, canary=KP.F8_NAN, device="cpu")
    return {"strided": (attn, dict(gap=4 + 24, behind=4 + 5 * 28, before=0, batch2_gap=4 + 8 * 28 + 27, tail=4 + 2 * 8 * 28)),
            "rows": (rows, dict(gap=24, behind=4 * 32, tail=7 * 32 + 63)),
            "rows [B, HW, C] fp32": (rows3, dict(gap=8, behind=6 * 12, tail=9 * 12)),
            "rows bytes": (rows8, dict(gap=16, behind=5 * 24)),
            "block": (block, dict(above=8, left=2 * 26 + 7, right=2 * 26 + 18, below=8 * 26 + 8, last=11 * 26 - 1)),
            "at": (at, dict(before=39, gap=40 + 12, other_rows=40 + 3 * 16, behind=40 + 5 * 16 + 3 * 16)),
            "at e4m3": (at8, dict(gap=12, behind=4 * 16))}


@pytest.mark.parametrize("name", list(_guards()))
def test_counts_tell_unwritten_from_overwritten(name):
    g, outside = _guards()[name]
    assert g.counts() == (int(g.inside.sum()), 0)          # nothing written yet: every inside element unwritten
    _fill(g)
    assert g.counts() == (0, 0)
    inside = g.inside.nonzero().flatten()
    for i in (inside[0], inside[len(inside) // 2], inside[-1]):
        g.bits[i] = g.canary                               # one inside element left unwritten
        assert g.counts() == (1, 0), (name, int(i))
        _fill(g)
    for where, i in outside.items():
        assert not g.inside[i], (name, where)
        keep = g.bits[i].clone()
        g.buf[i] = 1.0                                     # one stray store
        assert g.counts() == (0, 1), (name, where)
        g.bits[i] = keep
    assert g.counts() == (0, 0)


def test_a_canary_is_never_a_result():
    for dt in (torch.bfloat16, HF):
        assert torch.tensor([KP.CANARY16], dtype=torch.int16).view(dt).isnan().all()
    assert torch.tensor([KP.CANARY32], dtype=torch.int32).view(torch.float32).isnan().all()
    assert torch.tensor([KP.F8_NAN], dtype=torch.uint8).view(torch.float8_e4m3fn).float().isnan().all()
    assert KP.CANARY8 == 0xA5


def _geometry(g):
    return g.view.storage_offset(), tuple(g.view.stride()), g.bits.numel()


def test_geometry_of_existing_cases():
    """(offset in elements, strides, buffer length) of each family's output buffer for two of its cases, as before the shared pieces"""
    ed = torch.bfloat16
    # attention (attn_child._geom): "short Skv32 Sq77 S2": B 2, Sq 77, H 3, D 64, aligned: row pad 8, 3 extra rows, offset 0
    g = KP.Guarded.strided((2, 77, 3, 64), (16000, 200, 64, 1), 0, 32064, 16, dt=ed, device="cpu")
    assert _geometry(g) == (0, (16000, 200, 64, 1), 32064) and g.view.data_ptr() % 16 == g.buf.data_ptr() % 16
    # "flash64 D64 unaligned S1": Sq 129, row pad 4, offset 4 elements (an 8-byte-aligned base)
    g = KP.Guarded.strided((2, 129, 3, 64), (25872, 196, 64, 1), 4, 51812, 16, dt=ed, device="cpu")
    assert _geometry(g) == (4, (25872, 196, 64, 1), 51812) and g.view.data_ptr() - g.buf.data_ptr() == 8
    from tests.attn_child import _geom
    assert _geom(2, 77, 3, 64, 8, 3, 0) == ((2, 77, 3, 64), (16000, 200, 64, 1), 0, 32064)
    assert _geom(2, 129, 3, 64, 4, 3, 4) == ((2, 129, 3, 64), (25872, 196, 64, 1), 4, 51812)
    assert _geom(2, 77, 3, 64, 16, 40, 0) == ((2, 77, 3, 64), (24336, 208, 64, 1), 0, 48736)      # K / V of Skv 77
    # normalisation, row maps (_canary: 3 extra rows, 64 more elements): "ln C1032 ..." rows 3, ldy C + 8; "gn C320 HW3 ..." [2, 3, 320]
    g = KP.Guarded.rows((3, 1032), 1040, 16, extra_rows=3, tail=64, dt=ed, device="cpu")
    assert _geometry(g) == (0, (1040, 1), 6304)
    g = KP.Guarded.rows((2, 3, 320), 328, 16, extra_rows=3, tail=64, dt=ed, device="cpu")
    assert _geometry(g) == (0, (984, 328, 1), 3016)
    g = KP.Guarded.rows((5, 2), 2, 32, extra_rows=3, tail=64, device="cpu")                         # row_stats: fp32 [rows, 2]
    assert _geometry(g) == (0, (2, 1), 80) and g.view.dtype == torch.float32
    g = KP.Guarded.rows((1, 293), 293, 32, extra_rows=3, tail=64, device="cpu")                     # rowmap _flat_out(293, 32)
    assert _geometry(g) == (0, (293, 1), 1236)
    # convolution (conv_cases.alloc_out): "mask s2 cin8" M 24, N 40; "random 2x3 s1 all16 silu" M 12, N 72, fp32 or 16-bit
    g = CC.alloc_out(24, 40, ed, "cpu")
    assert _geometry(g) == (3592, (56, 1), 8512)
    g = CC.alloc_out(12, 72, torch.float32, "cpu")
    assert _geometry(g) == (5640, (88, 1), 12320) and g.view.dtype == torch.float32 and g.canary == KP.CANARY32
    # linear and four-wave GEMM children, "strided": M 257, N 324, 40 spare rows; M 8192, N 1536, 256 spare rows; 16 spare columns
    g = KP.Guarded.block(257, 324, 16, above=0, below=40, left=0, right=16, dt=ed, device="cpu")
    assert _geometry(g) == (0, (340, 1), 297 * 340)
    g = KP.Guarded.block(8192, 1536, 16, above=0, below=256, left=0, right=16, dt=ed, device="cpu")
    assert _geometry(g) == (0, (1552, 1), 8448 * 1552)
    # ... "c-remap": 3 batches of 77 rows with 154 foreign rows behind each, N 328
    g = KP.Guarded.strided((3, 77, 328), (231 * 328, 328, 1), 0, 3 * 231 * 328, 16, dt=ed, device="cpu")
    assert _geometry(g) == (0, (75768, 328, 1), 227304) and int(g.inside.sum()) == 231 * 328
    # W8A8 (gemm_f8_child._out): "x As 77x12x128 scale" ldc 20; "x As c-remap 40": segment 1 of 3 batches of 117 rows, ldc 268
    idx = row_offsets(77, 20)[:, None] + torch.arange(12)
    g = KP.Guarded.at(idx, 80 * 20 + 64, 16, base=0, dt=ed, device="cpu")
    assert g.bits.numel() == 1664 and g.ptr == g.buf.data_ptr() and idx[76, 11] == 1531
    idx = 20636 + row_offsets(120, 268, 40, 31356)[:, None] + torch.arange(260)
    g = KP.Guarded.at(idx, 354 * 268 + 64, 16, base=20636, dt=ed, device="cpu")
    assert g.bits.numel() == 94936 and g.ptr - g.buf.data_ptr() == 2 * 20636 and int(idx[119, 259]) == 20636 + 2 * 31356 + 39 * 268 + 259
    assert g.get().shape == (120, 260)


def test_nan_embedding():
    x = torch.arange(24.0).reshape(2, 3, 4)
    v = KP.nan_rows(x, 6, tail=64)                         # (norm_child._nan_rows: row gaps and 64 elements behind hold NaN)
    assert torch.equal(v, x) and tuple(v.stride()) == (18, 6, 1) and v.storage_offset() == 0
    flat = torch.as_strided(v, (6 * 6 + 64,), (1,), 0)
    assert int(flat.isnan().sum()) == 6 * 6 + 64 - 24
    vec = KP.nan_rows(torch.ones(1, 10), 10, tail=64)[0]   # a flat vector followed by 64 NaN
    assert vec.shape == (10,) and torch.as_strided(vec, (74,), (1,), 0)[10:].isnan().all()
    d, full = KP.nan_embed(x, x.stride(), 4096, 24 + 2 * 4096)   # (conv_child.nan_margins)
    assert torch.equal(d, x) and d.is_contiguous() and full[:4096].isnan().all() and full[-4096:].isnan().all()
    img = torch.ones(2, 5, 7, 8, dtype=HF)                 # (conv_cases.nan_embedded: pixel stride C + 24, first channel 8)
    view, full, first = CC.nan_embedded(img)
    assert (first, tuple(view.stride()), full.numel()) == (1128, (1120, 224, 32, 1), 4480) and view.storage_offset() == first
    assert int(full.isnan().sum()) == 4480 - img.numel() and torch.equal(view, img)
