"""CPU tests of tests/gemm_f8_bounds.py: the fp32 emulation of the W8A8 kernel (128-deep fp32 steps chained, the epilogue in the
code's order, one rounding to 16 bits, the e4m3 store), run on the GPU child's own operand generators at reduced M and N, stays well
inside the bound and is bit-equal in class 1; each planted mistake fails the class it belongs to -- bit inequality in class 1, ratio
> 1, a byte outside its interval or a row scale outside its allowance in class 2. Where a mutation passed, the inputs were changed,
never the bound."""
import pytest
import torch

from tests import gemm_bounds as GB
from tests import gemm_f8_bounds as FB
from tests.gemm_f8_child import CASES

EDS = [torch.bfloat16, torch.float16]
M, N, K = 100, 36, 256   # a gate batch boundary (77) inside a 16-row sub-tile; N % 8 == 4; two K-tiles


def _emu(o, ed, **kw):
    return FB.emulate(o["qa"], o["sa"], o["qw"], o["sw"], ed, bias=o["bias"], gate=o["gate"], rows_per_batch=o["rpb"],
                      residual=o["residual"], gelu=o.get("gelu", False), **kw)


def _ref(o):
    return FB.reference8(o["qa"], o["sa"], o["qw"], o["sw"], bias=o["bias"], gate=o["gate"], rows_per_batch=o["rpb"],
                         residual=o["residual"], gelu=o.get("gelu", False))


# ---- the pieces ------------------------------------------------------------------------------------------------------------------
def test_e4m3_round_is_torch_rne_on_fp32_values_and_saturates():
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(20000, generator=g) * 2.0 ** torch.randint(-12, 9, (20000,), generator=g).float(),
                   torch.arange(-256, 256).float() / 512, FB.from_bytes(torch.arange(256, dtype=torch.uint8)[:127]).float(),
                   torch.tensor([0.0, -0.0, 447.9, 448.0, 463.9])])
    x = x[x.abs() <= 464.0 - 1e-3]
    want = x.to(FB.F8).double()
    got = FB.e4m3_round(x.double())
    assert torch.equal(got, want)
    assert torch.equal(FB.e4m3_round(torch.tensor([500.0, -1e9], dtype=torch.float64)), torch.tensor([448.0, -448.0], dtype=torch.float64))
    # ties go to even in float64 too (2^-9 is the subnormal quantum; 17 sits between 16 and 18)
    assert FB.e4m3_round(torch.tensor([17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10], dtype=torch.float64)).tolist() == [16.0, 20.0, 0.0, 2.0 ** -8]
    assert FB.e4m3_round(torch.tensor([17.9, -17.9], dtype=torch.float64), toward_zero=True).tolist() == [16.0, -16.0]


def test_f8_nan_byte_and_gamma():
    assert torch.isnan(torch.tensor([FB.F8_NAN], dtype=torch.uint8).view(FB.F8).float()).all()
    assert FB.gamma8(128) == (1 + FB.STEP) * 2.0 ** -24 and FB.gamma8(6144) == (48 + FB.STEP) * 2.0 ** -24
    assert FB.STEP in (128, 256) and FB.EPI_OPS8 == 5 and FB.MULTI_CAP == 0.05


@pytest.mark.parametrize("rows,K", [(256, 128), (260, 256), (264, 1536), (300, 6144)])
def test_sparse_rows_visit_every_chunk_position_of_every_k_tile(rows, K):
    pos = FB.sparse_positions(rows, K)
    assert (pos.sort(1).values.diff(dim=1) > 0).all()                 # 16 distinct positions per row
    assert (pos[1:] != pos[:-1]).any(1).all()                         # ... that differ row by row
    assert len({tuple(r) for r in pos.tolist()}) >= min(rows, (K // 16) ** 2) // 2
    chunks = torch.zeros(K // 16, dtype=torch.bool)
    chunks[(pos // 16).reshape(-1)] = True
    assert chunks.all()                                               # every 16-byte chunk of every K-tile
    v = FB.from_bytes(FB.sparse_int(rows, K))
    assert ((v != 0).sum(1) == 16).all() and set(v.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}


def test_gather_rows_follows_the_remap():
    buf = torch.arange(3 * 117 * 10)
    got = FB.gather_rows(buf, 120, 4, 10, rpb=40, bstride=1170, base=770)
    assert got[0].tolist() == [770, 771, 772, 773] and got[39, 0] == 770 + 390 and got[40, 0] == 770 + 1170 and got[119, 3] == 770 + 2340 + 393


# ---- the correct emulation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ed", EDS)
@pytest.mark.parametrize("mirror", ["As", "Ws"])
@pytest.mark.parametrize("sub", ["scale", "epi"])
def test_class_1_preconditions_hold_and_the_emulation_is_bit_equal(ed, mirror, sub):
    o = FB.exact_operands(M, N, K, mirror, sub, ed)
    ref = FB.exact_reference(o, ed)   # (asserts ref.to(ed).double() == ref)
    acc = FB.from_bytes(o["qa"]) @ FB.from_bytes(o["qw"]).t()
    assert acc.abs().max() <= 256 and ref.abs().max() > 8
    assert FB.exact_off(_emu(o, ed), ref) == 0


@pytest.mark.parametrize("name", [n for n, s in CASES.items() if s["cls"] == "exact"])
def test_class_1_preconditions_of_every_committed_case(name):
    s = CASES[name]
    for ed in EDS:
        FB.exact_reference(FB.exact_operands(s["M"], s["N"], s["K"], s["mirror"], s["sub"], ed), ed)


@pytest.mark.parametrize("ed", EDS)
@pytest.mark.parametrize("form", ["", "bias", "bias+gelu", "gate", "gate+gelu"])
def test_class_2_correct_emulation_stays_below_half_the_bound(ed, form):
    o = FB.dense_operands(M, N, K, form, ed)
    ratio, rel = GB.check(_emu(o, ed), *_ref(o))
    assert ratio < 0.5, ratio
    assert rel < (4e-3 if ed == torch.bfloat16 else 6e-4)


@pytest.mark.parametrize("gelu", [False, True])
def test_e4m3_output_of_the_correct_emulation_is_accepted(gelu):
    o = FB.dense_operands(M, N, K, "bias+gelu" if gelu else "bias", torch.bfloat16)
    q, cs = _emu(o, torch.bfloat16, q=o)
    ref, e = _ref(o)
    r = FB.check_q(q, cs, ref, e, FB.out_scale64(o["a_l2"], o["w_norm_max"], o["bias_abs_max"]))
    assert r["scale_ratio"] <= 1.0 and r["outside"] == 0 and r["nan"] == 0 and r["multi"] <= FB.MULTI_CAP, r


def _q_operands(s):
    """the operands of a committed e4m3 case, as the child builds them"""
    if s["cls"] == "denseq":
        o = FB.dense_operands(s["M"], s["N"], s["K"], s["form"], torch.bfloat16)
        return o, _ref(o)
    o = FB.exact_operands(s["M"], s["N"], s["K"], s["mirror"], s["sub"], torch.bfloat16)
    FB.exact_q_operands(o)
    return o, _ref(o)


@pytest.mark.parametrize("name", [n for n, s in CASES.items() if s["cls"] == "denseq" or s.get("q")])
def test_multi_code_cap_holds_for_every_committed_e4m3_case(name):
    """a condition on the inputs, from the reference alone: at most 5 % of the intervals hold more than one code, and the
    Cauchy-Schwarz scale keeps every element inside e4m3's range"""
    o, (ref, e) = _q_operands(CASES[name])
    s64 = FB.out_scale64(o["a_l2"], o["w_norm_max"], o["bias_abs_max"])
    assert FB.multi_share(ref, e, s64) <= FB.MULTI_CAP
    assert ((ref.abs() + e) / s64[:, None]).max() < 448.0


# ---- the planted mistakes ------------------------------------------------------------------------------------------------------------
CLASS1_FAULTS = [("swap_chunks_a", "As", "scale"), ("swap_chunks_a", "Ws", "scale"), ("drop_last_ktile", "As", "scale"),
                 ("drop_last_ktile", "Ws", "epi"), ("a_scale_next_row", "As", "scale"), ("a_scale_next_row", "Ws", "scale"),
                 ("clamped_column", "As", "scale"), ("clamped_column", "Ws", "epi"), ("bias_twice", "As", "epi"),
                 ("gate_by_subtile", "As", "epi"), ("gate_by_subtile", "Ws", "epi"), ("residual_before_gate", "Ws", "epi")]


@pytest.mark.parametrize("ed", EDS)
@pytest.mark.parametrize("fault,mirror,sub", CLASS1_FAULTS)
def test_class_1_catches_each_planted_mistake(ed, fault, mirror, sub):
    o = FB.exact_operands(M, N, K, mirror, sub, ed)
    assert FB.exact_off(_emu(o, ed, fault=fault), FB.exact_reference(o, ed)) > 0


CLASS2_FAULTS = [("swap_chunks_a", ""), ("drop_last_ktile", "bias"), ("a_scale_next_row", ""), ("clamped_column", "bias"),
                 ("clamped_column", ""), ("bias_twice", "bias"), ("bias_twice", "bias+gelu"), ("gate_by_subtile", "gate"),
                 ("residual_before_gate", "gate"), ("residual_before_gate", "gate+gelu")]


@pytest.mark.parametrize("ed", EDS)
@pytest.mark.parametrize("fault,form", CLASS2_FAULTS)
def test_class_2_catches_each_planted_mistake(ed, fault, form):
    o = FB.dense_operands(M, N, K, form, ed)
    ratio, _ = GB.check(_emu(o, ed, fault=fault), *_ref(o))
    assert ratio > 1.0, ratio


def _remapped(o, seg):
    """o's A rows as segment `seg` of batches of 8 + 5 rows in a flat 0x7F buffer (lda = K + 16), base pointer at the segment"""
    segs, lda = (8, 5), K + 16
    rpb, base = segs[seg], (segs[0] * lda if seg else 0)
    nb = o["qa"].shape[0] // rpb
    buf = torch.full((nb * sum(segs) * lda + 256,), FB.F8_NAN, dtype=torch.uint8)
    idx = base + FB.row_offsets(nb * rpb, lda, rpb, sum(segs) * lda)[:, None] + torch.arange(K)
    buf[idx] = o["qa"]
    return buf, dict(M=nb * rpb, lda=lda, rpb=rpb, bstride=sum(segs) * lda, base=base)


@pytest.mark.parametrize("seg", [0, 1])
@pytest.mark.parametrize("mirror", ["As", "Ws"])
def test_a_remap_is_followed_and_ignoring_the_batch_stride_is_caught(seg, mirror):
    ed = torch.bfloat16
    o = FB.exact_operands(40, N, K, mirror, "scale", ed)
    ref = FB.exact_reference(o, ed)
    buf, rm = _remapped(o, seg)
    assert FB.exact_off(FB.emulate(buf, o["sa"], o["qw"], o["sw"], ed, a_remap=rm), ref) == 0
    assert FB.exact_off(FB.emulate(buf, o["sa"], o["qw"], o["sw"], ed, a_remap=rm, fault="a_remap_no_stride"), ref) > 0
    d = FB.dense_operands(40, N, K, "", ed)
    buf, rm = _remapped(d, seg)
    ratio, _ = GB.check(FB.emulate(buf, d["sa"], d["qw"], d["sw"], ed, a_remap=rm, fault="a_remap_no_stride"), *_ref(d))
    assert ratio > 1.0


@pytest.mark.parametrize("gelu", [False, True])
def test_e4m3_output_catches_the_missing_1p1_and_rounding_toward_zero(gelu):
    o = FB.dense_operands(M, N, K, "bias+gelu" if gelu else "bias", torch.bfloat16)
    ref, e = _ref(o)
    s64 = FB.out_scale64(o["a_l2"], o["w_norm_max"], o["bias_abs_max"])
    q, cs = _emu(o, torch.bfloat16, q=o, fault="no_1p1")
    assert FB.check_q(q, cs, ref, e, s64)["scale_ratio"] > 1.0
    q, cs = _emu(o, torch.bfloat16, q=o, fault="e4m3_toward_zero")
    r = FB.check_q(q, cs, ref, e, s64)
    assert r["scale_ratio"] <= 1.0 and r["outside"] > 0.3 * q.numel(), r
    # the class 1 operands through the e4m3 output: the interval is a single code nearly everywhere, and still catches it
    x = FB.exact_operands(M, N, K, "As", "scale", torch.bfloat16)
    FB.exact_q_operands(x)
    ref, e = _ref(x)
    s64 = FB.out_scale64(x["a_l2"], x["w_norm_max"], 0.0)
    r = FB.check_q(*_emu(x, torch.bfloat16, q=x), ref, e, s64)
    assert r["scale_ratio"] <= 1.0 and r["outside"] == 0 and r["nan"] == 0 and r["multi"] <= FB.MULTI_CAP, r
    assert FB.check_q(*_emu(x, torch.bfloat16, q=x, fault="e4m3_toward_zero"), ref, e, s64)["outside"] > 0
    assert FB.check_q(*_emu(x, torch.bfloat16, q=x, fault="swap_chunks_a"), ref, e, s64)["outside"] > 0


def test_every_fault_of_the_module_is_exercised():
    used = {f for f, *_ in CLASS1_FAULTS} | {f for f, _ in CLASS2_FAULTS} | {"a_remap_no_stride", "no_1p1", "e4m3_toward_zero"}
    assert used == set(FB.FAULTS)
