"""The bounds and restatements of tests/rowmap_bounds.py, checked on the CPU: a torch fp32 emulation of each bound-class kernel's
arithmetic in its own order (csrc/misc.hip) stays under its bound on the inputs the GPU cases use (the all-values sweeps, the softmax
rows, the timestep cases; CPU-seeded draws of the same distributions for the random ones), and every injected fault lands above 1.0
on the case built to expose it. The layout restatements are run against coded inputs with each pair of axes exchanged and the two
column orders exchanged: every exchange changes the output. Ratios are printed (pytest -s)."""
import itertools
import math

import numpy as np
import pytest
import torch

from tests import rowmap_bounds as RB
from tests.rowmap_child import CASES, TS

F32 = torch.float32
DTS = (torch.bfloat16, torch.float16)
LOG2E = float(np.float32(1.4426950408889634))


def r32(t):
    return t.to(F32)


def mul32(a, b):
    return (a.double() * b.double()).to(F32)


def exp_fast(a):
    """__expf: v_exp_f32 of fl(a * log2e) (emulated correctly rounded)"""
    return torch.exp2(mul32(a, torch.tensor(LOG2E, dtype=F32)).double()).to(F32)


def rcp32(a):
    return (1.0 / a.double()).to(F32)


# ---- activations --------------------------------------------------------------------------------------------------------------
def emulate_act(kind, x, fault=None):
    """x fp32 -> fp32 value before the store; fault: c17 (1.7 for 1.702) | swap_gelu (erf <-> tanh)"""
    if fault == "swap_gelu":
        kind = {"gelu": "gelu_new", "gelu_new": "gelu"}[kind]
    if kind == "silu":
        return mul32(x, rcp32(r32(1.0 + exp_fast(-x))))
    if kind == "quick_gelu":
        c = np.float32(1.7 if fault == "c17" else 1.702)
        a = mul32(torch.tensor(-c, dtype=F32), x)
        return (x.double() / r32(1.0 + exp_fast(a)).double()).to(F32)
    if kind == "gelu":
        xc = x.clamp(-8.0, 8.0)
        t = mul32(xc, xc).double()
        q = (np.float32(0.0010127116) * t + np.float32(-0.10676638)).to(F32).double()
        q = mul32((q * t + np.float32(-2.3011315)).to(F32), xc)
        return mul32(x, rcp32(r32(1.0 + torch.exp2(q.double()).to(F32))))
    if kind == "gelu_new":
        c1 = torch.tensor(RB.TANH_C1, dtype=F32)
        cube = mul32(mul32(mul32(c1, x), x), x)
        u = mul32(torch.tensor(RB.TANH_C0, dtype=F32), r32(x + cube))
        return mul32(x, rcp32(r32(1.0 + exp_fast(mul32(torch.tensor(-2.0), u)))))
    raise ValueError(kind)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", ["silu", "quick_gelu", "gelu", "gelu_new"])
def test_activation_emulation_inside_the_bound(kind, dt):
    x = RB.sweep16(dt)
    ref, e = RB.act(kind, x.double())
    ratio = RB.check(emulate_act(kind, x.float()).to(dt), ref, e)
    print(f"{kind} {dt}: err/bound {ratio:.3f}")
    assert ratio < 1.0


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("out_dt", ["same", F32])
def test_silu_fp32_forms_inside_the_bound(dt, out_dt):
    x = RB.sweep32(dt)
    if out_dt == F32:
        big = torch.finfo(F32).max
        x = torch.cat([x, torch.tensor([big, -big])])
    ref, e = RB.act("silu", x.double())
    ratio = RB.check(emulate_act("silu", x).to(dt if out_dt == "same" else F32), ref, e)
    print(f"silu f32 -> {out_dt} ({dt}): err/bound {ratio:.3f}")
    assert ratio < 1.0


def _gated_input(dt, F=64):
    a = RB.sweep16(dt)
    a = torch.cat([a, torch.zeros((-a.numel()) % F, dtype=dt)]).reshape(-1, F)
    g = torch.Generator().manual_seed(3)
    b = 2.0 * torch.randn(a.shape, generator=g)
    b = torch.where(a.float().abs() > 128.0, torch.full_like(b, -0.5), b).to(dt)
    return a, b


def emulate_gated(kind, x, ldx, F, fault=None):
    """x fp32 [rows, ldx] (NaN in the gap past 2F); fault: halves | half_ld (second half at ldx / 2) | c17 | swap_gelu"""
    a, b = x[:, :F], x[:, F:2 * F]
    if fault == "halves":
        a, b = b, a
    elif fault == "half_ld":
        b = x[:, ldx // 2:ldx // 2 + F]
    return mul32(emulate_act(kind, a, fault), b)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", ["silu", "quick_gelu", "gelu", "gelu_new"])
def test_gated_emulation_and_faults(kind, dt):
    F = 64
    a, b = _gated_input(dt, F)
    ldx = 2 * F + 16
    x = torch.full((a.shape[0], ldx), float("nan"))
    x[:, :F], x[:, F:2 * F] = a.float(), b.float()
    ref, e = RB.gated(kind, a.double(), b.double())
    good = RB.check(emulate_gated(kind, x, ldx, F).to(dt), ref, e)
    bad = {f: RB.check(emulate_gated(kind, x, ldx, F, f).to(dt), ref, e) for f in ("halves", "half_ld")}
    print(f"gated {kind} {dt}: err/bound {good:.3f}; faults {bad}")
    assert good < 1.0
    assert all(v > 1.0 for v in bad.values()), bad
    # at ldx == 2F the two independent quantities coincide: half_ld is invisible there (why the ldx > 2F case exists)
    same = RB.check(emulate_gated(kind, x[:, :2 * F].contiguous(), 2 * F, F, "half_ld").to(dt), ref, e)
    assert same == good


@pytest.mark.parametrize("dt", DTS)
def test_quick_gelu_constant_fault(dt):
    x = RB.sweep16(dt)
    ref, e = RB.act("quick_gelu", x.double())
    bad = RB.check(emulate_act("quick_gelu", x.float(), "c17").to(dt), ref, e)
    print(f"quick_gelu 1.7 for 1.702 {dt}: err/bound {bad:.2f}")
    assert bad > 1.0


@pytest.mark.parametrize("kind", ["gelu", "gelu_new"])
def test_gelu_forms_exchanged(kind):
    """must fail at the fp16 bound; the bf16 ratio is reported and, thanks to the negative tail of the all-values sweep (where the
    two forms differ by 4.7e-4 around x = -2.9 and the value itself is 5e-3), also lands above 1"""
    got = {}
    for dt in DTS:
        x = RB.sweep16(dt)
        ref, e = RB.act(kind, x.double())
        got[dt] = RB.check(emulate_act(kind, x.float(), "swap_gelu").to(dt), ref, e)
    print(f"{kind} computed as the other GELU: fp16 err/bound {got[torch.float16]:.2f}, bf16 {got[torch.bfloat16]:.2f}")
    assert got[torch.float16] > 1.0
    assert got[torch.bfloat16] > 1.0


# ---- softmax_rows -------------------------------------------------------------------------------------------------------------
def emulate_softmax(x, dt, fault=None):
    """x fp32 [rows, n]; fault: max_skips_last | drop_wave | rounded_sum | no_max"""
    rows, n = x.shape
    n4 = n // 4
    m = (x[:, :-4] if fault == "max_skips_last" else x).amax(1, keepdim=True)
    if fault == "no_max":
        m = torch.zeros_like(m)
    E = exp_fast(r32(x - m))
    Es = E.to(dt).float() if fault == "rounded_sum" else E
    trips = (n4 + 255) // 256
    c = torch.zeros(rows, trips * 256, 4)
    c[:, :n4] = Es.reshape(rows, n4, 4)
    c = r32(r32(r32(c[..., 0] + c[..., 1]) + c[..., 2]) + c[..., 3]).reshape(rows, trips, 256)
    s = torch.zeros(rows, 256)
    for t in range(trips):
        s = r32(s + c[:, t])          # (adding the 0 of an idle thread changes nothing)
    s = s.reshape(rows, 4, 64)
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = r32(s + s[..., lanes ^ o])
    red = s[..., 0].clone()
    if fault == "drop_wave":
        red[:, 3] = 0.0
    S = r32(r32(red[:, 0] + red[:, 1]) + r32(red[:, 2] + red[:, 3]))[:, None]
    return mul32(Es, rcp32(S)).to(dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [4, 1020, 1028, 16384])
def test_softmax_emulation_inside_the_bound(n, dt):
    x = RB.softmax_rows_input(n, "cpu")
    ref, e = RB.softmax(x)
    ratio = RB.check(emulate_softmax(x, dt), ref, e)
    print(f"softmax n{n} {dt}: err/bound {ratio:.3f}")
    assert ratio < 1.0


@pytest.mark.parametrize("fault", ["max_skips_last", "drop_wave", "no_max"])
def test_softmax_faults_fail_the_bound(fault):
    """the maximum of the spanning row sits in the last four-wide chunk (leaving it out overflows the exponentials); a dropped wave
    loses a quarter of every sum; without the subtraction the -10000 row is 0 / 0"""
    x = RB.softmax_rows_input(1028, "cpu")
    ref, e = RB.softmax(x)
    for dt in DTS:
        bad = RB.check(emulate_softmax(x, dt, fault), ref, e)
        print(f"softmax {fault} {dt}: err/bound {bad:.2f}")
        assert bad > 1.0


def test_softmax_sum_of_rounded_probabilities():
    """65535 keys whose exponential 0.99 * 2^-25 rounds to an fp16 zero under one peak: the rounded sum is 1 instead of 1.0019.
    Outside the fp16 bound; bf16 has no subnormal range within reach and cannot see this fault (its ratio is printed)."""
    n = 65536
    x = torch.full((1, n), math.log(0.99 * 2.0 ** -25))
    x[0, 7] = 0.0
    ref, e = RB.softmax(x)
    good = RB.check(emulate_softmax(x, torch.float16), ref, e)
    bad = RB.check(emulate_softmax(x, torch.float16, "rounded_sum"), ref, e)
    bf = RB.check(emulate_softmax(RB.softmax_rows_input(1028, "cpu"), torch.bfloat16, "rounded_sum"), *RB.softmax(RB.softmax_rows_input(1028, "cpu")))
    print(f"softmax rounded_sum: fp16 err/bound {good:.3f} -> {bad:.2f}; bf16 on the case rows {bf:.3f}")
    assert good < 1.0 and bad > 1.0


# ---- timestep_embedding -------------------------------------------------------------------------------------------------------
def emulate_timestep(t, n, dim, group, flip, shift, scale, period, dt, fault=None):
    """[n, dim]; fault: swap | no_shift | dim_denominator | index | pad"""
    half = dim // 2
    j = torch.arange(half, dtype=F32)
    den = r32(torch.tensor(float(dim if fault == "dim_denominator" else half)) - (0.0 if fault == "no_shift" else np.float32(shift)))
    ex = (mul32(-torch.log(torch.tensor(period, dtype=F32)), j).double() / den.double()).to(F32)
    i = torch.arange(n)
    tt = t[(i // group) % t.numel() if fault == "index" else i % t.numel()]
    arg = mul32(torch.tensor(scale, dtype=F32), mul32(tt[:, None], torch.exp(ex)[None]))
    sn, cs = torch.sin(arg), torch.cos(arg)
    if fault == "swap":
        sn, cs = cs, sn
    parts = [cs, sn] if flip else [sn, cs]
    if dim & 1:
        parts.append(torch.full((n, 1), 2.0 ** -20 if fault == "pad" else 0.0))
    return torch.cat(parts, 1).to(dt)


def _temb_args(s):
    t = torch.tensor(s.get("t", TS), dtype=F32)
    return t, s.get("n", t.numel()), s["dim"], s.get("group", 1), s["flip"], s["shift"], s.get("scale", 1.0), s.get("period", 10000.0)


@pytest.mark.parametrize("name", [k for k, v in CASES.items() if v[0] == "temb"])
def test_timestep_emulation_inside_the_bound(name):
    t, n, dim, group, flip, shift, scale, period = _temb_args(CASES[name][1])
    ref, e = RB.timestep(t, n, dim, flip, shift, scale, period)
    for dt in DTS:
        ratio = RB.check(emulate_timestep(t, n, dim, group, flip, shift, scale, period, dt), ref, e)
        print(f"{name} {dt}: err/bound {ratio:.3f}")
        assert ratio < 1.0


@pytest.mark.parametrize("fault,name", [("swap", "temb dim320 shift0 flip"), ("no_shift", "temb dim64 shift1"),
                                        ("dim_denominator", "temb dim320 shift0 flip"), ("index", "temb dim64 group6 t_count<n"),
                                        ("pad", "temb dim321 odd shift1 flip")])
def test_timestep_faults_fail_the_bound(fault, name):
    t, n, dim, group, flip, shift, scale, period = _temb_args(CASES[name][1])
    ref, e = RB.timestep(t, n, dim, flip, shift, scale, period)
    for dt in DTS:
        bad = RB.check(emulate_timestep(t, n, dim, group, flip, shift, scale, period, dt, fault), ref, e)
        print(f"timestep {fault} {dt}: err/bound {bad:.2f}")
        assert bad > 1.0


# ---- axpby, cfg_axpby, latent_dist --------------------------------------------------------------------------------------------
def _cfg_input(gs, n=3000):
    g = torch.Generator().manual_seed(int(gs * 10) + 1)
    x = 3.0 * torch.randn(n, generator=g)
    u = torch.randn(n, generator=g)
    t = u * (1 + 2.0 ** -10 * torch.randn(n, generator=g)) if gs == 1.0 else u + 0.3 * torch.randn(n, generator=g)
    if gs == 0.0:
        u = x * (1 + 2.0 ** -12 * torch.randn(n, generator=g))
    coef = torch.tensor((1.0127, -0.0423) if gs else (1.5, -1.5))
    return x, u, t, coef


def emulate_cfg(x, u, t, coef, gs, fault=None):
    """fault: swap (eu and et exchanged) | wrong_half (the guidance pulls towards eu)"""
    if fault == "swap":
        u, t = t, u
    gs32 = torch.tensor(gs, dtype=F32)
    gdn = r32(t + mul32(gs32, r32(u - t))) if fault == "wrong_half" else r32(u + mul32(gs32, r32(t - u)))
    return r32(mul32(coef[0], x) + mul32(coef[1], gdn))


@pytest.mark.parametrize("gs", [0.0, 1.0, 7.5])
def test_cfg_axpby_emulation_and_faults(gs):
    x, u, t, coef = _cfg_input(gs)
    ref, e = RB.cfg_axpby(x, u, t, coef, gs)
    good = RB.check(emulate_cfg(x, u, t, coef, gs), ref, e)
    fused = RB.check((coef[0].double() * x.double() + coef[1].double() * r32(u + mul32(torch.tensor(gs), r32(t - u))).double()).to(F32), ref, e)
    bad = {f: RB.check(emulate_cfg(x, u, t, coef, gs, f), ref, e) for f in ("swap", "wrong_half")}
    print(f"cfg gs{gs:g}: err/bound {good:.3f} (fused {fused:.3f}); faults {bad}")
    assert good < 1.0 and fused < 1.0
    assert all(v > 1.0 for v in bad.values()), bad


def test_axpby_emulation_inside_the_bound():
    g = torch.Generator().manual_seed(2)
    x = 3.0 * torch.randn(3000, generator=g)
    for coef, y in (((0.25, -1.5), torch.randn(3000, generator=g)), ((1.5, -1.5), x * (1 + 2.0 ** -12 * torch.randn(3000, generator=g)))):
        c = torch.tensor(coef)
        ref, e = RB.axpby(x, y, c)
        sep = RB.check(r32(mul32(c[0], x) + mul32(c[1], y)), ref, e)
        fma = RB.check((c[0].double() * x.double() + mul32(c[1], y).double()).to(F32), ref, e)
        bad = RB.check(r32(mul32(c[1], x) + mul32(c[0], y)), ref, e)
        print(f"axpby {coef}: err/bound {sep:.3f} (one product fused {fma:.3f}); coefficients exchanged {bad:.1f}")
        assert sep < 1.0 and fma < 1.0 and bad > 1.0


def emulate_latent(m, B, L, noise, scale, fault=None):
    """fault: clip (bounds exchanged) | full_exp (exp(lv) for exp(0.5 lv))"""
    mu, lv = RB.nchw(m, B, L), RB.nchw(m[:, L:], B, L)
    lv = lv.clamp_min(20.0).clamp_max(-30.0) if fault == "clip" else lv.clamp_min(-30.0).clamp_max(20.0)
    std = exp_fast(lv if fault == "full_exp" else mul32(torch.tensor(0.5), lv))
    return lv, mul32(r32(mu + mul32(std, noise)), torch.tensor(scale, dtype=F32))


def test_latent_dist_emulation_and_faults():
    B, L, HW = 2, 4, 67
    g = torch.Generator().manual_seed(8)
    m = torch.cat([3.0 * torch.randn(B * HW, L, generator=g), 20.0 * torch.randn(B * HW, L, generator=g),
                   torch.full((B * HW, 4), float("nan"))], 1)
    m[0, L:2 * L] = torch.tensor([-30.0, 20.0, -30.5, 20.5])
    noise = torch.randn(B, L, HW, generator=g)
    ref, e = RB.latent_sample(m, B, L, noise, 0.18215)
    lv, out = emulate_latent(m, B, L, noise, 0.18215)
    good = RB.check(out, ref, e)
    assert RB.exact_off(lv.contiguous(), RB.latent_moments(m, B, L, 0.18215)[1]) == 0
    print(f"latent sample: err/bound {good:.3f}")
    assert good < 1.0
    for fault in ("clip", "full_exp"):
        lvf, bad = emulate_latent(m, B, L, noise, 0.18215, fault)
        r = RB.check(bad, ref, e)
        print(f"latent {fault}: err/bound {r:.2e}")
        assert r > 1.0
    assert RB.exact_off(emulate_latent(m, B, L, noise, 0.18215, "clip")[0].contiguous(), RB.latent_moments(m, B, L, 0.18215)[1]) > 0


# ---- layout kernels: coded inputs, every exchange detected --------------------------------------------------------------------
def _swaps(axes):
    for i, j in itertools.combinations(range(len(axes)), 2):
        o = list(axes)
        o[i], o[j] = o[j], o[i]
        yield tuple(o)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,C,H,W,p", [(2, 16, 6, 10, 2), (2, 3, 8, 12, 4), (2, 16, 8, 12, 4)])
def test_patchify_exchanges_are_detected(B, C, H, W, p, dt):
    """unique codes (B C H W <= CODE_PRIME): each of the 15 axis exchanges and the (py, px, c) column order changes the output"""
    assert B * C * H * W <= RB.CODE_PRIME
    x = RB.codes(B * C * H * W, dt).float().reshape(B, C, H, W)
    want = RB.patchify(x, p, dt)
    assert RB.exact_off(want.float().to(dt), want) == 0 and want.unique().numel() == want.numel()   # the codes survive the rounding
    for order in list(_swaps(RB.PATCH_AXES)) + [("b", "ty", "tx", "py", "px", "c")]:
        assert RB.exact_off(RB.patchify(x, p, dt, order), want) > 0, order


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,C,H,W,p", [(2, 16, 6, 10, 2), (2, 3, 8, 12, 4), (2, 16, 8, 12, 4)])
def test_unpatchify_exchanges_are_detected(B, C, H, W, p, dt):
    rows, K = B * (H // p) * (W // p), C * p * p
    x = RB.codes(rows * K, dt).reshape(rows, K)
    want = RB.unpatchify(x, B, C, H, W, p)
    for order in _swaps(RB.UNPATCH_AXES):
        assert RB.exact_off(RB.unpatchify(x, B, C, H, W, p, order=order), want) > 0, order
    assert RB.exact_off(RB.unpatchify(x, B, C, H, W, p, cols=("c", "py", "px")), want) > 0
    # and the pair is a round trip only through the column permutation: patchify's (c, py, px) rows fed to unpatchify as they are
    # do NOT give the image back
    img = RB.codes(B * C * H * W, dt).float().reshape(B, C, H, W)
    assert RB.exact_off(RB.unpatchify(RB.patchify(img, p, dt), B, C, H, W, p), img) > 0
    assert RB.exact_off(RB.unpatchify(RB.patchify(img, p, dt), B, C, H, W, p, cols=("c", "py", "px")), img) == 0


@pytest.mark.parametrize("dt", DTS)
def test_split_concat_and_add_nchw_exchanges_are_detected(dt):
    B, S1, S2, C = 3, 7, 9, 16
    allv = RB.codes(B * (S1 + S2) * 3 * C, dt)
    x, y = allv[:B * S1 * 3 * C].reshape(B, S1, 3 * C), allv[B * S1 * 3 * C:].reshape(B, S2, 3 * C)
    want = RB.split_concat(x, y)
    assert sum(RB.exact_off(a, b) for a, b in zip(RB.split_concat(x, y, ("c", "i")), want)) > 0
    assert sum(RB.exact_off(a, b) for a, b in zip((want[1], want[0], want[2]), want)) > 0
    Bn, Cn, HW = 3, 8, 100
    r = RB.codes(Bn * Cn * HW, dt).float().reshape(Bn, Cn, HW)
    x0 = torch.zeros(Bn, HW, Cn, dtype=dt)
    want = RB.add_nchw(x0, r)
    assert RB.exact_off(want.permute(0, 2, 1).contiguous(), r.to(dt)) == 0   # x = 0: the output is the residual's code
    for order in ((0, 1, 2), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        assert RB.exact_off(RB.add_nchw(x0, r, order), want) > 0, order


def test_inputs_cover_what_the_issue_names():
    for dt in DTS:
        s = RB.sweep16(dt).float()
        every = torch.arange(0, 0x8000).to(torch.int16).view(dt).float()
        every = every[torch.isfinite(every) & (every <= 16.0)]
        got = set(s.tolist())
        assert set(every.tolist()) <= got and set((-every).tolist()) <= got          # every value of [-16, 16]
        assert (s == 0).sum() >= 2 and torch.signbit(s[s == 0]).any()                   # both zeros
        assert s.max() == torch.finfo(dt).max and s.min() == -torch.finfo(dt).max      # the largest finite values
        assert s[(s.abs() > 88.8) & (s.abs() < 128)].numel() > 0 and s[(s < -103.98) & (s > -128)].numel() > 0   # past over- / underflow
    assert all(RB.CODE_PRIME % q for q in range(2, 174))                               # CODE_PRIME is prime
    assert RB.CODE_BASE[torch.float16] + RB.CODE_PRIME < 0x7C00 and RB.CODE_BASE[torch.bfloat16] + RB.CODE_PRIME < 0x7F80
