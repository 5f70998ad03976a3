"""CPU: the convolution references, bounds and selector inputs of tests/conv_bounds.py / tests/conv_cases.py against an emulation of
the kernels' gather IN ITS OWN ORDER (csrc/gemm.hip issue_tile: per K-tile of 64, per lane chunk of 8 channels, the running
(tap, channel) state of common.h conv_k_init / conv_k_next for both K orders, iy = oy * stride + ky - pad, the upsample shift, zero
fill, addresses formed on the flat NaN-guarded allocation) feeding fp32 sums in 32-deep steps. On scaled-down cases of every kind the
emulation is exact on the selectors and inside the bound on random data; each injected fault fails an exact selector or lands at
least 10x outside the bound (the factor tests/test_norm_bounds.py uses) on the case built for it."""
import pytest
import torch

from tests import conv_bounds as CB
from tests import conv_cases as CC
from tests.conv_cases import Case

ED = torch.bfloat16


def k_init(kb64, kt, cg8, Cin):
    if kb64:
        cb = kt // 9
        return kt - cb * 9, cb * 64 + cg8
    ch = kt * 64 + cg8
    return ch // Cin, ch % Cin


def k_next(kb64, Cin, tap, ch):
    if kb64:
        tap += 1
        if tap == 9:
            tap, ch = 0, ch + 64
        return tap, ch
    ch += 64
    while ch >= Cin:
        ch, tap = ch - Cin, tap + 1
    return tap, ch


def emulate(case, d, fault=None):
    """the kernel's output [M, Cout] for build()'s operands, computed the kernel's way (with one fault injected when named)"""
    s, up, br = CC.GEOMS[case.geom]
    up = int(up)
    pad = 0 if br else 1
    B, Hs, Ws, Cin, N = case.B, case.H, case.W, case.Cin, case.Cout
    K, lda = 9 * Cin, Cin + CC.X_GAP
    Ho, Wo, M = d["Ho"], d["Wo"], d["M"]
    flat = d["x_full"].float()
    if fault == "pad_all_round":
        pad = 1
    kb64_walk = case.kb64 and fault != "kb64_plain_walk"
    m = torch.arange(M)
    b, rem = m // (Ho * Wo), m % (Ho * Wo)
    oy, ox = rem // Wo, rem % Wo
    base = d["x_first"] + b * (Hs * Ws * lda)
    Hin, Win = Hs << up, Ws << up
    nt = (K + 63) // 64
    if fault == "drop_last_ktile":
        nt = K // 64
    w = d["w_dev"].float()
    acc = torch.zeros(M, N)
    state = [k_init(kb64_walk, 0, cg * 8, Cin) for cg in range(8)]
    for kt in range(nt):
        a = torch.zeros(M, 64)
        for cg in range(8):
            tap, ch = state[cg]
            assert (tap, ch) == k_init(kb64_walk, kt, cg * 8, Cin)   # (the running state equals a fresh start at every K-tile)
            state[cg] = k_next(kb64_walk, Cin, tap, ch)
            if kt * 64 + cg * 8 >= K:
                continue
            ky, kx = tap // 3, tap % 3
            if fault == "kykx_swapped":
                ky, kx = kx, ky
            iy = oy * s + ky - pad + (1 if fault == "stride2_origin" and s == 2 else 0)
            ix = ox * s + kx - pad
            ok = (iy >= 0) & (iy < Hin + (1 if fault == "bottom_row_next_item" else 0)) & (ix >= 0) & (ix < Win)
            sy, sx = (iy, ix) if fault == "no_upsample_shift" else (iy >> up, ix >> up)
            c0 = ch + (8 if fault == "neighbour_chunk" and cg == 3 else 0)
            off = (base + (sy * Ws + sx) * lda + c0).clamp(0, flat.numel() - 8)
            chunk = flat[off[:, None] + torch.arange(8)[None, :]]
            a[:, cg * 8:cg * 8 + 8] = torch.where(ok[:, None], chunk, torch.zeros(()))
        wt = torch.zeros(N, 64)
        kw = min(64, K - kt * 64)
        wt[:, :kw] = w[:, kt * 64:kt * 64 + kw]
        for ks in range(2):   # two 32-deep MFMA steps per K-tile, fp32 accumulator
            acc = acc + a[:, ks * 32:ks * 32 + 32] @ wt[:, ks * 32:ks * 32 + 32].t()
    v = acc
    if d["bias"] is not None:
        v = v + d["bias"]
    if d["rowbias"] is not None:
        v = v + d["rowbias"][m // ((Hs * Ws) if fault == "rowbias_source_pixels" else (Ho * Wo))]
    if d["residual"] is not None:
        v = v + d["residual"].float()
    if fault == "silu_before_scale" and d["silu"]:
        v = v * torch.sigmoid(v)
    v = v * torch.tensor(d["out_scale"], dtype=torch.float32)
    if d["silu"] and fault != "silu_before_scale":
        v = v * torch.sigmoid(v)
    return v if d["out_f32"] else v.to(ED)


def _small():
    c = {}
    for g in CC.GEOMS:
        for kb in (False, True):
            o = "kb64" if kb else "plain"
            cin = 128 if kb else 64   # (at Cin = 64 the two K orders are the same order)
            c[f"coded {g} {o}"] = Case("coded", 2, 7, 5, cin, 40, g, kb, ())
            c[f"mask {g} {o}"] = Case("mask", 2, 5, 7, cin, 32, g, kb, ())
    for g in ("s1", "s2up", "s2br"):
        c[f"coded {g} cin40"] = Case("coded", 2, 5, 3, 40, 72, g, False, ())
        c[f"coded {g} cin8"] = Case("coded", 2, 5, 3, 8, 24, g, False, ())
    for g in CC.GEOMS:
        if g != "s2br":
            c[f"coded 1x1 {g}"] = Case("coded", 2, 1, 1, 64, 24, g, g == "s2", ())
        c[f"mask 2x3 {g}"] = Case("mask", 2, 2, 3, 64, 24, g, g == "s1up", ())
    c["coded cin192 kb64"] = Case("coded", 2, 3, 5, 192, 40, "s2", True, ())
    c["random s1 bias"] = Case("random", 2, 7, 5, 64, 40, "s1", False, ("bias",))
    c["random s2 all16 kb64"] = Case("random", 2, 7, 5, 128, 40, "s2", True, ("bias", "rowbias", "r16", "scale"))
    c["random s1up rowbias+r32"] = Case("random", 2, 5, 3, 64, 40, "s1up", False, ("rowbias", "r32"))
    c["random s2br silu"] = Case("random", 2, 7, 5, 64, 40, "s2br", True, ("bias", "silu"))
    c["random s2up f32 out"] = Case("random", 2, 5, 3, 64, 40, "s2up", False, ("bias", "r32", "scale", "f32"))
    c["random s2 cin40"] = Case("random", 2, 7, 5, 40, 40, "s2", False, ("bias", "r16"))
    c["random s1 silu after scale"] = Case("random", 2, 7, 5, 128, 40, "s1", True, ("bias", "rowbias", "scale", "silu"))
    c["random 2x3 s2br kb64 rowbias+r32 f32 out"] = Case("random", 2, 2, 3, 128, 24, "s2br", True, ("rowbias", "r32", "f32"))
    return c


SMALL = _small()


def _judge(name, case, fault=None):
    d = CC.build(name, case, ED, "cpu")
    return CC.judge(case, d, emulate(case, d, fault))


@pytest.mark.parametrize("name", list(SMALL))
def test_emulated_gather_is_exact_on_selectors_and_inside_the_bound(name):
    r = _judge(name, SMALL[name])
    print(f"{name:<28} err/bound {r['ratio']:.3f} mismatch {r['mismatch']}")
    assert r["mismatch"] in (None, 0) and r["ratio"] < 1.0, (name, r)


# fault -> the cases built for it (name in SMALL)
FAULTS = {
    "pad_all_round": ["mask s2br plain", "coded s2br kb64"],                 # padding all round where bottom / right was asked
    "no_upsample_shift": ["coded s1up plain", "mask s2up kb64"],             # the upsample shift dropped
    "bottom_row_next_item": ["coded s1 plain", "mask s1 kb64"],              # the bottom padding row reads the next item's first row
    "kb64_plain_walk": ["coded s1 kb64", "coded cin192 kb64"],               # kb64 weights walked in plain order
    "kykx_swapped": ["coded s1 plain", "mask s2 plain"],                     # ky and kx exchanged
    "stride2_origin": ["coded s2 plain", "mask s2br kb64"],                  # the stride-2 origin off by one
    "drop_last_ktile": ["coded s1 cin40"],                                   # the last K-tile (K = 360: 40 elements) dropped
    "rowbias_source_pixels": ["random s2 all16 kb64"],                       # rowbias indexed by source instead of output pixels
    "neighbour_chunk": ["coded s1 plain", "coded s2up kb64"],                # one 8-channel chunk taken from the neighbouring chunk
    "silu_before_scale": ["random s1 silu after scale"],                     # SiLU applied before out_scale instead of after it
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_injected_gather_faults_are_rejected(fault):
    for name in FAULTS[fault]:
        r = _judge(name, SMALL[name], fault)
        print(f"fault {fault:<22} on {name:<24} err/bound {r['ratio']:.1f}  exact mismatches {r['mismatch']}")
        if r["mismatch"] is not None:
            assert r["mismatch"] > 0, (fault, name, r)
        else:
            assert r["ratio"] >= 10.0, (fault, name, r)


def test_coded_input_separates_neighbours():
    """the coded value differs between any two pixels within two steps in y and x, between channels c and c + 1 / + 8 / + 64, and
    between batch items; it is a non-zero integer of magnitude <= 126"""
    x = CC.coded_x(3, 13, 11, 192, "cpu")
    assert x.abs().min() >= 1 and x.abs().max() <= 126 and torch.equal(x, x.round())
    assert torch.equal(x.to(torch.bfloat16).float(), x) and torch.equal(x.to(torch.float16).float(), x)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if (dy, dx) != (0, 0):
                a = x[:, max(0, dy):13 + min(0, dy), max(0, dx):11 + min(0, dx)]
                b = x[:, max(0, -dy):13 + min(0, -dy), max(0, -dx):11 + min(0, -dx)]
                assert (a != b).all(), (dy, dx)
    for dc in (1, 8, 64):
        assert (x[..., dc:] != x[..., :-dc]).all(), dc
    assert (x[0] != x[1]).all() and (x[1] != x[2]).all() and (x[0] != x[2]).all()


def test_im2col_equals_the_documented_gather():
    """im2col() (interpolate / pad / unfold only) equals the gather csrc/gemm.hip issue_tile documents, element for element, on every
    geometry at odd sizes, 1 x 1 and 2 x 3"""
    for g, (s, up, br) in CC.GEOMS.items():
        for (H, W) in ((1, 1), (2, 3), (5, 7), (4, 4)):
            if br and (H < 2 or W < 2):
                continue
            x = CC.coded_x(2, H, W, 8, "cpu")
            a, Ho, Wo = CB.im2col(x, s, up, br)
            pad, u = (0 if br else 1), int(up)
            for b in range(2):
                for oy in range(Ho):
                    for ox in range(Wo):
                        for tap in range(9):
                            iy, ix = oy * s + tap // 3 - pad, ox * s + tap % 3 - pad
                            inside = 0 <= iy < (H << u) and 0 <= ix < (W << u)
                            want = x[b, iy >> u, ix >> u] if inside else torch.zeros(8)
                            assert torch.equal(a[(b * Ho + oy) * Wo + ox, tap].float(), want), (g, H, W, b, oy, ox, tap)


def test_kb64_packing_round_trip():
    w = torch.arange(6 * 9 * 128, dtype=torch.float32).view(6, 9 * 128)
    assert torch.equal(CB.from_kb64(CB.to_kb64(w)), w)
    p = CB.to_kb64(w).view(6, 2, 9, 64)
    assert p[3, 1, 4, 5] == w.view(6, 9, 128)[3, 4, 64 + 5]


def test_direct_kernel_bounds_hold_for_fp32_chains_and_reject_a_dropped_tap():
    """the three direct kernels' references against plain fp32 torch convolutions of the same rounded operands (inside the bound), and
    against the same with one tap's weights zeroed (>= 10x outside)"""
    g = torch.Generator().manual_seed(5)
    F = torch.nn.functional
    x = torch.randn(2, 4, 6, 7, generator=g)
    w = CC.exact16(torch.randn(16, 4, 3, 3, generator=g) / 6)
    bias, sc = torch.randn(16, generator=g), torch.tensor([0.7])
    wk = w.permute(2, 3, 1, 0).reshape(36, 16).to(ED)
    ref, e = CB.conv_in3x3_reference(x, wk, bias, sc, ED)
    for drop, want in ((False, "in"), (True, "out")):
        w2 = w.clone()
        if drop:
            w2[:, :, 2, 0] = 0
        o = F.conv2d((x * sc).to(ED).float(), w2, bias, padding=1).permute(0, 2, 3, 1).reshape(-1, 16)
        r16, r32 = CB.check(o.to(ED), ref, e)[0], CB.check(o, ref, e)[0]
        print(f"conv_in dropped tap {drop}: err/bound 16-bit {r16:.2f} fp32 {r32:.2f}")
        assert (r16 < 1 and r32 < 1) if want == "in" else (r16 >= 10 and r32 >= 10)
    xo = CC.exact16(torch.randn(2, 6, 7, 64, generator=g)).to(ED)
    wo = CC.exact16(torch.randn(4, 3, 3, 64, generator=g) / 24)
    bo = torch.randn(4, generator=g)
    ref, e = CB.conv_out3x3_reference(xo, wo.reshape(4, -1).to(ED), bo)
    for drop in (False, True):
        w2 = wo.clone()
        if drop:
            w2[:, 0, 1] = 0
        o = F.conv2d(xo.float().permute(0, 3, 1, 2), w2.permute(0, 3, 1, 2), bo, padding=1)
        r = CB.check(o, ref, e)[0]
        print(f"conv_out dropped tap {drop}: err/bound {r:.2f}")
        assert r >= 10 if drop else r < 1
    x1 = torch.randn(2, 4, 5, 3, generator=g)
    w1 = CC.exact16(torch.randn(8, 4, generator=g))
    ref, e = CB.conv1x1_nchw_reference(x1, w1.to(ED), bo.repeat(2), 0.13, ED)
    for drop in (False, True):
        w2 = w1.clone()
        if drop:
            w2[:, 3] = 0
        o = F.conv2d((x1 * torch.tensor(0.13)).to(ED).float(), w2[:, :, None, None], bo.repeat(2))
        r = CB.check(o, ref, e)[0]
        print(f"conv1x1 dropped channel {drop}: err/bound {r:.2f}")
        assert r >= 10 if drop else r < 1
