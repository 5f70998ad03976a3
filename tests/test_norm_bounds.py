"""The elementwise fp64 bounds of tests/norm_bounds.py, checked on the CPU against emulations of the normalisation kernels' fp32
arithmetic in their own order (csrc/norm.hip, csrc/fused_ops.hip): the shifted one-pass row statistics with their per-lane chains
and the 64-lane butterfly, the GroupNorm block partials (pixels per thread, LDS adds over ppp, channel adds over the group) in fp32
followed by the double finalize and fma(x, scale, shift), and the adaLN modulation rows. On scaled-down cases of every input kind the
emulation stays inside the bound; each injected fault lands outside it by at least the factor stated, on the case built to expose
it -- among them today's GroupNorm arithmetic before this bound (unshifted sums of x and x^2) at |mean| / std >= 1000."""
import numpy as np
import pytest
import torch

from tests import norm_bounds as NB

F32 = torch.float32


def r32(t):
    return t.to(F32)


def fma32(a, b, c):
    """fp32 fma: the exact a * b + c (in float64: exact for fp32 products) rounded once"""
    return (a.double() * b.double() + c.double()).to(F32)


# ---- row kernels (row_norm_kernel's forms: LayerNormRows, RowStats, AdaLNRows; fused_adaln_scale_residual_kernel) ----------------
def row_moments(x, n_ch, fault=None):
    """x fp32 [rows, C]: (mean, rstd-input var) of the shifted one-pass statistics: lane l owns chunks l + 64 i (i < NCH), chains
    of 8 per chunk in order, then the butterfly over 64 lanes; fault: unshifted | drop_last"""
    rows, C = x.shape
    cv = C // 8
    K = torch.zeros(rows, 1, dtype=F32) if fault == "unshifted" else x[:, :1].clone()
    s = torch.zeros(rows, 64, dtype=F32)
    q = torch.zeros(rows, 64, dtype=F32)
    for i in range(n_ch):
        cc = torch.arange(64) + 64 * i   # (vectorised over the lanes)
        ok = cc < cv
        if fault == "drop_last":
            ok = ok & (cc != cv - 1)
        for j in range(8):
            d = r32(x[:, cc.clamp(max=cv - 1) * 8 + j] - K)
            s = torch.where(ok[None], r32(s + d), s)
            q = torch.where(ok[None], fma32(d, d, q), q)
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = r32(s + s[:, lanes ^ o])
        q = r32(q + q[:, lanes ^ o])
    invC = torch.tensor(1.0 / C, dtype=F32)
    m = r32(s[:, :1] * invC)
    var = torch.clamp(r32(r32(q[:, :1] * invC) - r32(m * m)), min=0.0)
    return r32(K + m), var


def rstd32(var, eps, fault=None):
    n_eps = torch.tensor(NB.fp32(eps), dtype=F32)
    if fault == "eps_outside":
        return r32(1.0 / r32(r32(var.sqrt()) + n_eps))
    return r32(1.0 / r32(r32(var + n_eps).double().sqrt()))


def emulate_layernorm(x, gamma, beta, eps, out_dt, fault=None):
    C = x.shape[1]
    mean, var = row_moments(x, NB.nch("layernorm", C), fault)
    if fault == "n_minus_1":
        var = r32(var * C / (C - 1))
    rstd = rstd32(var, eps, fault)
    z = r32(r32(x - mean) * rstd)
    g, b = gamma, beta
    if fault == "chunk":   # gamma / beta of the neighbouring 8-channel chunk
        g, b = torch.roll(g, 8), torch.roll(b, 8)
    return fma32(z, g[None], b[None]).to(out_dt)


def emulate_adaln(x, scale, shift, rpb, eps, rows_per_wave, out_dt, fault=None):
    rows, C = x.shape
    mean, var = row_moments(x, NB.nch("adaln", C))
    rstd = rstd32(var, eps)
    z = r32(r32(x - mean) * rstd)
    row = torch.arange(rows)
    b = (row - row % rows_per_wave) // rpb if fault == "modrow" else row // rpb
    return fma32(z, r32(1 + scale[b, :C]), shift[b, :C]).to(out_dt)


# ---- GroupNorm: gn_partial_kernel + gn_finalize_kernel + scale_shift_act_kernel -------------------------------------------------
def emulate_groupnorm(x, gamma, beta, groups, eps, silu, out_dt, fault=None):
    """x fp32 values [B, HW, C]; fault: unshifted (the kernels before the bound) | n_minus_1 | eps_outside"""
    B, HW, C = x.shape
    cv, ppp, _, _, ppb, nblk = NB.gn_geom(HW, C)
    cpg = C // groups
    K = torch.zeros(B, 1, C, dtype=F32) if fault == "unshifted" else x[:, :1, torch.arange(C) // cpg * cpg].clone()
    xp = torch.zeros(B, nblk * ppb, C, dtype=F32)
    xp[:, :HW] = x
    present = torch.zeros(nblk * ppb, dtype=torch.bool)
    present[:HW] = True
    xb = xp.reshape(B, nblk, NB.GN_ITERS_STATS, ppp, C)   # pixel = blk * ppb + it * ppp + pl
    pb = present.reshape(nblk, NB.GN_ITERS_STATS, ppp)
    s = torch.zeros(B, nblk, ppp, C, dtype=F32)
    q = torch.zeros(B, nblk, ppp, C, dtype=F32)
    for it in range(NB.GN_ITERS_STATS):
        ok = pb[None, :, it, :, None]
        d = r32(xb[:, :, it] - K[:, None])
        s = torch.where(ok, r32(s + d), s)
        q = torch.where(ok, fma32(d, d, q), q)
    a = torch.zeros(B, nblk, C, dtype=F32)
    dq = torch.zeros(B, nblk, C, dtype=F32)
    for pl in range(ppp):   # LDS: per channel over the pixel slots
        a, dq = r32(a + s[:, :, pl]), r32(dq + q[:, :, pl])
    ga = torch.zeros(B, nblk, groups, dtype=F32)
    gq = torch.zeros(B, nblk, groups, dtype=F32)
    ar, qr = a.reshape(B, nblk, groups, cpg), dq.reshape(B, nblk, groups, cpg)
    for c in range(cpg):    # per group over its channels
        ga, gq = r32(ga + ar[..., c]), r32(gq + qr[..., c])
    # finalize in double: 8 strided partial sums per group, then the 8 in order
    S = torch.zeros(B, groups, dtype=torch.float64)
    Q = torch.zeros(B, groups, dtype=torch.float64)
    for j in range(8):
        sj = torch.zeros(B, groups, dtype=torch.float64)
        qj = torch.zeros(B, groups, dtype=torch.float64)
        for i in range(j, nblk, 8):
            sj, qj = sj + ga[:, i].double(), qj + gq[:, i].double()
        S, Q = S + sj, Q + qj
    n = HW * cpg
    m = S / n
    var = (Q / n - m * m).clamp(min=0.0)
    if fault == "n_minus_1":
        var = var * n / (n - 1)
    Kg = K[:, 0, ::cpg].double()
    e32 = NB.fp32(eps)
    mean = r32(Kg + m)
    rstd = r32(1.0 / (var.sqrt() + e32)) if fault == "eps_outside" else r32(1.0 / (var + e32).sqrt())
    mean_c, rstd_c = mean.repeat_interleave(cpg, 1), rstd.repeat_interleave(cpg, 1)
    sc = r32(gamma[None] * rstd_c)
    sh = r32(beta[None] - r32(mean_c * sc))
    o = fma32(x, sc[:, None], sh[:, None])
    if silu:
        o = r32(o * r32(1.0 / r32(1.0 + torch.exp(-o.double()).to(F32))))
    return o.to(out_dt)


def _gn_case(B, HW, C, groups, r, dt, seed, outlier=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, HW, C, generator=g) + r
    if outlier is not None:
        x[:, outlier[0], outlier[1]] = r + 50.0
    x = x.to(dt).float() if dt != F32 else x
    gamma = (1 + 0.3 * torch.randn(C, generator=g)).float()
    beta = (0.3 * torch.randn(C, generator=g)).float()
    return x, gamma, beta


GN_CASES = [   # (B, HW, C, groups, r, input dtype, outlier)
    (2, 96, 64, 32, 0.0, torch.bfloat16, None), (1, 300, 320, 32, 16.0, torch.bfloat16, None),
    (1, 200, 320, 32, 256.0, torch.bfloat16, (0, 0)), (1, 1024, 320, 32, 1000.0, F32, None),
    (1, 256, 320, 32, 4096.0, F32, (5, 7)), (2, 37, 64, 1, 256.0, torch.float16, None), (1, 40, 2056, 8, 0.0, F32, (0, 0)),
]


@pytest.mark.parametrize("B,HW,C,groups,r,dt,outlier", GN_CASES)
@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_emulation_inside_the_bound(B, HW, C, groups, r, dt, outlier, silu):
    x, gamma, beta = _gn_case(B, HW, C, groups, r, dt, B * HW + C + int(r), outlier)
    for out_dt in (torch.bfloat16, torch.float16):
        out = emulate_groupnorm(x, gamma, beta, groups, 1e-5, silu, out_dt)
        ref, e = NB.groupnorm(x, gamma, beta, groups, 1e-5, silu, L=NB.chain_gn_split(HW, C, groups))
        ratio, _ = NB.check(out, ref, e)
        assert ratio < 1.0, (out_dt, ratio)


@pytest.mark.parametrize("r,dt,factor", [(1000.0, F32, 100.0), (4096.0, F32, 1000.0), (1000.0, torch.float16, 100.0)])
def test_unshifted_groupnorm_sums_fail_the_bound(r, dt, factor):
    """The GroupNorm arithmetic before the bound (sums of x and x^2, var = q / n - mean^2) at |mean| / std = r on the UNet's geometry
    (HW = 1024, C = 320, 32 groups): the variance drowns in the fp32 roundoff of sum x^2 ~ n r^2."""
    x, gamma, beta = _gn_case(1, 1024, 320, 32, r, dt, 7)
    ref, e = NB.groupnorm(x, gamma, beta, 32, 1e-5, False, L=NB.chain_gn_split(1024, 320, 32))
    good, _ = NB.check(emulate_groupnorm(x, gamma, beta, 32, 1e-5, False, torch.float16), ref, e)
    bad, _ = NB.check(emulate_groupnorm(x, gamma, beta, 32, 1e-5, False, torch.float16, fault="unshifted"), ref, e)
    print(f"r = {r}: shifted err/bound {good:.3f}, unshifted {bad:.1f}")
    assert good < 1.0
    assert bad > factor


@pytest.mark.parametrize("fault,factor", [("n_minus_1", 10.0), ("eps_outside", 100.0)])
def test_groupnorm_statistics_faults_fail_the_bound(fault, factor):
    """N - 1 on a 4 x 4 group (n = 16: 1 / (2n) = 3 % against fp16's 2^-10); eps outside the square root on a near-constant set with
    var ~ eps"""
    if fault == "n_minus_1":
        x, gamma, beta = _gn_case(1, 4, 64, 16, 0.0, F32, 3)
    else:
        g = torch.Generator().manual_seed(4)
        x = (3.0 + 3e-3 * torch.randn(1, 64, 64, generator=g)).float()
        gamma, beta = torch.ones(64), torch.zeros(64)
    HW, C = x.shape[1], x.shape[2]
    groups = 16 if fault == "n_minus_1" else 32
    ref, e = NB.groupnorm(x, gamma, beta, groups, 1e-5, False, L=NB.chain_gn_split(HW, C, groups))
    good, _ = NB.check(emulate_groupnorm(x, gamma, beta, groups, 1e-5, False, torch.float16), ref, e)
    bad, _ = NB.check(emulate_groupnorm(x, gamma, beta, groups, 1e-5, False, torch.float16, fault=fault), ref, e)
    print(f"{fault}: err/bound {good:.3f} -> {bad:.1f}")
    assert good < 1.0 and bad > factor


def _ln_case(rows, C, r, dt, seed, kind="random"):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) + r
    if kind == "outlier0":
        x[:, 0] = r + 50.0
    elif kind == "outlier_last":
        x[:, -3] = r + 50.0
    elif kind == "pm":
        x = r + torch.where(torch.arange(C) % 2 == 0, 1.5, -1.5).expand(rows, C).clone()
    elif kind == "const":
        x = torch.full((rows, C), r + 0.75)
    elif kind == "near_const":
        x = r + 2.0 ** -7 * torch.randint(0, 2, (rows, C), generator=g).float()   # (var = 2^-16 ~ eps, exact in bf16 at r = 1)
    x = x.to(dt).float() if dt != F32 else x
    gamma = (1 + 0.3 * torch.randn(C, generator=g)).float()
    beta = (0.3 * torch.randn(C, generator=g)).float()
    return x, gamma, beta


LN_CASES = [(5, 1024, 0.0, torch.bfloat16, "random"), (3, 1032, 16.0, torch.bfloat16, "outlier0"),
            (4, 1544, 256.0, torch.bfloat16, "outlier_last"), (3, 2560, 1000.0, F32, "random"), (2, 520, 4096.0, F32, "outlier0"),
            (3, 64, 0.0, torch.bfloat16, "pm"), (2, 64, 3.0, torch.bfloat16, "const"), (3, 1024, 1.0, torch.bfloat16, "near_const"),
            (2, 1536, 1000.0, torch.float16, "random")]


@pytest.mark.parametrize("rows,C,r,dt,kind", LN_CASES)
def test_layernorm_emulation_inside_the_bound(rows, C, r, dt, kind):
    x, gamma, beta = _ln_case(rows, C, r, dt, rows * C + int(r), kind)
    ref, e = NB.layernorm(x, gamma, beta, 1e-5, NB.chain_rows("layernorm", C))
    for out_dt in (torch.bfloat16, torch.float16):
        ratio, _ = NB.check(emulate_layernorm(x, gamma, beta, 1e-5, out_dt), ref, e)
        assert ratio < 1.0, (out_dt, ratio)


@pytest.mark.parametrize("fault,case,factor", [
    ("unshifted", (3, 1024, 4096.0, F32, "random"), 10.0),
    ("n_minus_1", (4, 16, 0.0, F32, "random"), 10.0),
    ("eps_outside", (3, 1024, 1.0, torch.bfloat16, "near_const"), 10.0),
    ("drop_last", (4, 1032, 0.0, torch.bfloat16, "outlier_last"), 10.0),
    ("chunk", (4, 1024, 0.0, torch.bfloat16, "random"), 10.0)])
def test_layernorm_faults_fail_the_bound(fault, case, factor):
    rows, C, r, dt, kind = case
    x, gamma, beta = _ln_case(rows, C, r, dt, 11, kind)
    ref, e = NB.layernorm(x, gamma, beta, 1e-5, NB.chain_rows("layernorm", C))
    good, _ = NB.check(emulate_layernorm(x, gamma, beta, 1e-5, torch.float16), ref, e)
    bad, _ = NB.check(emulate_layernorm(x, gamma, beta, 1e-5, torch.float16, fault=fault), ref, e)
    print(f"{fault}: err/bound {good:.3f} -> {bad:.1f}")
    assert good < 1.0 and bad > factor


@pytest.mark.parametrize("rpb,rows_per_wave,C", [(77, 4, 1024), (154, 4, 1536), (4250, 4, 1024), (77, 2, 2560)])
def test_adaln_modulation_rows(rpb, rows_per_wave, C):
    """adaLN at a rows_per_batch that is not a multiple of the kernel's ROWS (4, or 2 for C > 1536): the emulation is inside the
    bound; taking the modulation row of the wave's first row (the neighbouring batch item's for the rows past the boundary) is far
    outside."""
    rows = 2 * rpb + 3
    g = torch.Generator().manual_seed(rpb)
    x = torch.randn(rows, C, generator=g).to(torch.bfloat16).float()
    scale = (0.5 * torch.randn(3, C + 8, generator=g)).float()
    shift = (2.0 * torch.randn(3, C + 8, generator=g)).float()
    ref, e = NB.adaln(x, scale, shift, rpb, 1e-6, NB.chain_rows("adaln", C))
    good, _ = NB.check(emulate_adaln(x, scale, shift, rpb, 1e-6, rows_per_wave, torch.bfloat16), ref, e)
    bad, _ = NB.check(emulate_adaln(x, scale, shift, rpb, 1e-6, rows_per_wave, torch.bfloat16, fault="modrow"), ref, e)
    print(f"rpb {rpb}: err/bound {good:.3f} -> {bad:.1f}")
    assert good < 1.0 and bad > 10.0


def test_e4m3_conversion_is_rne_with_subnormals():
    """the CPU side of the exact quantize_rows check: RNE, ties to even, the subnormal range (spacing 2^-9), 448 the largest"""
    v = np.array([448.0, 1.0 + 2 ** -4, 1.0 + 3 * 2 ** -4, 2 ** -9, 1.5 * 2 ** -9, 2 ** -10, 2 ** -6 - 2 ** -10, 0.0, -3.0],
                 dtype=np.float32)
    got = NB.e4m3_value(torch.from_numpy(NB.e4m3_rne(v))).numpy()
    assert list(got) == [448.0, 1.0, 1.25, 2 ** -9, 2 ** -8, 0.0, 2 ** -6, 0.0, -3.0]


def test_quantize_rows_exact_emulation():
    """qs * q of the exact emulation is inside the e4m3 part of the bound (half a spacing of |x / qs| + the scale's roundings),
    and the row maximum lands on 448 exactly"""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(6, 256, generator=g) * 3
    x[1] = 0.0
    x[2, :] = 1e-4 * torch.randn(256, generator=g)
    x[2, 5] = 30.0
    x = x.to(torch.bfloat16)
    q, qs = NB.quantize_rows_exact(x)
    ref = x.double()
    ratio, _, _, nan = NB.check_f8(q, qs, None, ref, torch.zeros_like(ref))
    assert ratio < 1.0 and nan == 0
    assert (q[1] == 0).all()
    big = NB.e4m3_value(q).abs().amax(1)
    assert (big[[0, 2, 3, 4, 5]] == 448.0).all()
