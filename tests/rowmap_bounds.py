"""Float64 bounds and exact restatements for the row-map and layout kernels: the 15 small kernels of csrc/misc.hip outside the three
direct convolutions, plus split_concat of csrc/fused_ops.hip. Plain Python + torch; runs on whatever device the tensors live on. The
sibling of tests/gemm_bounds.py and tests/norm_bounds.py, with their constants (imported, not restated): u32 = 2^-24,
u_out = 2^-7 (bf16) / 2^-10 (fp16), ACT_REL = 2^-20, GELU_ERF_ABS = 3e-5, EXP_REL = 2^-21 (v_exp_f32), RCP = 2 u32 (v_rcp_f32).

Two classes.

EXACT class -- the kernel moves data or does one fp32 operation and one rounding, so the WHOLE output buffer must equal a plain torch
restatement bit for bit (exact_off() counts the elements that do not): copy_rows, cast_rows (RNE, as torch's .to()), patchify,
unpatchify, split_concat, embed_tokens (fl16(float(tok) + float(pos)); without a position table float(tok) + 0, which turns -0
into +0), add_nchw (fl16(float(x) + r) on 16-bit rows, fl32(x + r) on fp32 rows), mask_to_bias (fl(fl(1 - m) * -10000): a product
followed by nothing, so -ffp-contract=fast has nothing to fuse) and latent_dist's mean, clipped logvar and noise == NULL sample
(fl(mu * out_scale): mu + 0 is exact).
The layout kernels get CODED inputs (codes()): element i of an input carries the 16-bit pattern BASE + i, a distinct finite positive
value of the build's element type that survives the 16-bit rounding unchanged. The small cases keep every coded tensor below
CODE_PRIME = 30011 elements, so every element is unique and exchanging any two axes, or the (c, py, px) and (py, px, c) column
orders, changes the output (tests/test_rowmap_bounds.py does each exchange). The large grid-stride cases cannot be numbered by a
16-bit value; there element i carries i mod CODE_PRIME (a prime, so no axis length divides it): they are there for the stride
expression and the ragged last trip, the small ones for the orders.

BOUND class -- fp32 arithmetic with approximated transcendentals or contractions. Each output element is held to
|out - ref| <= u |ref| + (1 + u) e + floor, ref the float64 value computed from the exact operands the kernel reads, e derived
below, u = u_out and floor = 2^-24 (fp16's subnormal spacing) for a 16-bit store, u = 2 u32 (one fp32 ulp) and floor = 0 for an
fp32 store. check() returns the worst err / bound over the WHOLE output (a non-finite output -> inf; err = bound = 0 passes).
The inputs are exact, so no slope term (gemm_bounds.SLOPE) enters anywhere.

  * Activations (silu_kernel's four dtype forms, activation_kernel, gated_activation_kernel). Three of the forms are
    value = x * sigmoid(-a) with E = __expf(a) = v_exp_f32(fl(a * log2e)) and value' = x * v_rcp(1 + E) (quick-GELU: a true
    division): SiLU a = -x, quick-GELU a = fl(-1.702f x), tanh-GELU a = -2 u, u = fl(0.79788456f * (x + 0.044715f x^3)). The
    constant part -- v_exp_f32, 1 + E, the reciprocal, the product: 8 + 1 + 2 + 1 u32 -- is ACT_REL |value| (16 u32). The
    ARGUMENT's own roundings are relative to a, so they grow with |a|: the product with log2e and log2e's fp32 representation
    (2 u32 |a|), quick-GELU's product 1.702f x (+1), tanh-GELU's three products, one sum and the outer product (+5); the reference
    uses the fp32 constants, so their representation is no error. dE / E = K_ARG u32 |a| reaches the value through
    d value / value = (1 - sigmoid(-a)) dE / E = sigmoid(a) dE / E -- nothing where the sigmoid saturates at 1, everything in the
    negative tail, where value ~ x e^-|a|. Hence e = |value| (ACT_REL + K_ARG u32 |a| sigmoid(a)), K_ARG = 2 / 3 / 7. Where E
    overflows (a > 88.7) the kernel returns -0 for a true value below |x| 2^-128, and where 1 / (1 + E) is subnormal v_rcp_f32
    may flush it: an absolute (|x| + 1) 2^-126, which only an fp32 store can see.
    erf-GELU is x * sigmoid(p(x)) with a fitted quintic, 2.6e-5 absolute on Phi: e = GELU_ERF_ABS max(|x|, 1); the reference is
    0.5 x erfc(-x / sqrt 2), exact in the tails.
    gated: out = fl(act(a) * b): e = |b| e_act(a) + u32 |ref|.
    The tails separate the forms. erf- and tanh-GELU differ by up to 4.7e-4, an even function of x peaking near |x| = 2.9: on the
    positive side that is 1.6e-4 of the value and invisible to a 16-bit store, on the negative side the value itself is 5e-3, so
    on the all-values sweep an erf kernel computing the tanh form lands at 5.3 x the fp16 bound and 3.5 x the bf16 bound (the
    other way round: 400 x and more). 1.7 for 1.702 moves quick-GELU's negative tail by 0.002 |x| relatively: 10 x the fp16
    bound, 1.9 x the bf16 bound (tests/test_rowmap_bounds.py prints these). Both element types separate both faults.
  * softmax_rows: p_j = fl(E_j * inv), E_j = __expf(d_j), d_j = fl(x_j - m) (m the exact row maximum), inv = 1.0f / s.
      - the exponential: fl(x - m), the product with log2e and log2e's representation are each u32 relative to d, so
        dE_j / E_j = 3 u32 |d_j| + EXP_REL: it grows with |x - m|, 240 u32 at the 80-below-the-peak keys;
      - the row sum, in the kernel's structure: a thread adds the four exponentials of a chunk (3 additions) to its running sum,
        once per trip, ceil(n / 1024) trips; a 64-lane butterfly (6); the four wave partials (2): L = ceil(n / 1024) + 11
        additions of positive terms, |s' - S| <= gamma(L) S + sum_j dE_j. Relative to S the second term is the p-weighted mean
        of dE_j / E_j over the row (computed, not bounded by its maximum: the far keys weigh nothing);
      - the reciprocal (RCP: the division is correctly rounded or a v_rcp_f32) and the product: 3 u32;
      - the absolute floor 2^-24 of check(): fp16's subnormal spacing; it also covers v_exp_f32 flushing E_j below 2^-126.
    e = 1.01 p (dE_j / E_j + mean_p(dE / E) + gamma(L) + 3 u32). An all -inf row makes the float64 reference 0 / 0 and is left
    out; so is every NaN input.
    Normalising by the sum of the ROUNDED exponentials moves s by at most one half-ulp of the element type, relatively -- under
    u_out = 2 u by construction -- unless the keys are in fp16's subnormal range, where each loses up to 2^-25 absolutely:
    65536 keys just below 2^-25 under one peak shift s by 2^-9 and land at ~2 x the fp16 bound. bf16 has no such range and cannot
    see this fault (at most 0.75 of its bound).
  * timestep_embedding: exponent = fl(fl(-logf(max_period) * j) / fl(half - freq_shift)), freq = expf(exponent),
    arg = fl(scale * fl(t * freq)), then sinf / cosf and the 16-bit store. Every libm call is taken at <= 2 ulp = 4 u32 relative
    (the device library documents 1). The exponent carries logf (4) + product (1) + difference (1) + division (1) = K_EXP = 7 u32,
    relative; expf turns that into K_EXP u32 |exponent| relative on freq and adds its own 4; the two products add 2:
    |d arg| <= |arg| u32 (K_ARG_T + K_EXP |exponent|), K_ARG_T = 6. sin and cos move by at most |d arg| and add their own
    4 u32 (|value| <= 1): e = |d arg| + 4 u32. At scale = 1000 arguments reach 1e5 and e ~ 1e-1: the bound is honestly loose
    there. The pad column of an odd dim has ref = 0, e = 0 and is additionally required to be +0 bit for bit.
    dim < 4 with freq_shift = 1 divides 0 by 0 (in the reference model too); that input is left out.
  * axpby / cfg_axpby (fp32 out): which products fuse is the compiler's choice (-ffp-contract=fast), so no bit equality.
    out = a x + b y: every evaluation order rounds at most twice values of magnitude <= |a x| + |b y|:
    e = 2 u32 (|a x| + |b y|). cfg: g = u + gs (t - u): fl(t - u) (u32 |t - u|, times |gs|), the product (u32 |gs (t - u)|), the
    sum (u32 (|u| + |gs (t - u)|)): e_g = u32 (3 |gs| |t - u| + |u|); e = |b| e_g + 2 u32 (|a x| + |b| (|g| + e_g)).
  * latent_dist sample = fl((mu + __expf(0.5 lv) * noise) * out_scale): std carries u32 |0.5 lv| twice (log2e product and
    constant) + EXP_REL, the product with the noise and the sum one u32 each of |std noise| resp. |mu| + |std noise|, the
    scale one more: e = |out_scale| (|std noise| (2 u32 |0.5 lv| + EXP_REL + u32) + 2 u32 (|mu| + |std noise|)).

No route log: these launchers have no picker. The template form (silu's IN_F32 / OUT_F32, add_nchw's XF32) and the runtime `kind`
follow from the arguments of the call, so a case names its form by what it passes.
"""
import math

import numpy as np
import torch

from tests import bound_pieces as BP
from tests.bound_pieces import U32, U_OUT, exact_off, fp32  # noqa: F401  (U_OUT, exact_off: for the importers of this module)
from tests.gemm_bounds import ACT_REL, GELU_ERF_ABS
from tests.norm_bounds import EXP_REL, RCP, gamma

K_ARG = {"silu": 2, "quick_gelu": 3, "gelu_new": 7}
K_EXP, K_ARG_T, SINCOS_ABS = 7, 6, 4 * U32
F32_TINY = 2.0 ** -126
QUICK = float(np.float32(1.702))
TANH_C0, TANH_C1 = float(np.float32(0.7978845608028654)), float(np.float32(0.044715))
CODE_PRIME = 30011
CODE_BASE = {torch.bfloat16: 0x0080, torch.float16: 0x0400}   # the first normal pattern; BASE + CODE_PRIME stays finite
KINDS = {"quick_gelu": 0, "gelu": 1, "silu": 2, "gelu_new": 3}
BLOCK = 256
GRID_CAP = {"silu": 4096, "activation": 4096, "gated_activation": 4096, "embed_tokens": 4096, "copy_rows": 4096, "cast_rows": 4096,
            "axpby": 2048, "cfg_axpby": 2048, "mask_to_bias": 1024, "patchify": 8192, "unpatchify": 8192, "latent_dist": 8192,
            "split_concat": 8192}   # the block cap of each grid-stride launcher (csrc/misc.hip, csrc/fused_ops.hip)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def codes(numel, dt, device="cpu"):
    """element i = the 16-bit pattern BASE + (i mod CODE_PRIME) viewed as dt: distinct finite positive values (unique while
    numel <= CODE_PRIME)"""
    idx = torch.arange(numel, device=device) % CODE_PRIME
    return (idx + CODE_BASE[dt]).to(torch.int16).view(dt)


def sweep16(dt, device="cpu", limit=128.0):
    """every representable value of dt with |x| <= limit -- subnormals and both zeros included: all of [-16, 16] and on out past
    where __expf overflows (88.7) and underflows (-87.3 normal, -103.9 subnormal) -- plus the largest finite values, padded with
    zeros to a multiple of 8"""
    pos = torch.arange(0, 0x7C00 if dt == torch.float16 else 0x7F80, device=device).to(torch.int16).view(dt)
    pos = pos[pos.float() <= limit]
    big = torch.tensor([torch.finfo(dt).max], dtype=dt, device=device)
    v = torch.cat([pos, -pos, big, -big])
    pad = (-v.numel()) % 8
    return torch.cat([v, torch.zeros(pad, dtype=dt, device=device)])


F32_EDGES = (88.0, 88.5, 88.72284, 88.8, 89.0, 87.0, 87.33655, 87.5, 103.0, 103.9721, 104.0, 110.0, 52.14, 17.3287, 1e-30, 1e-40)


def sweep32(dt, device="cpu"):
    """the fp32-input forms: sweep16 widened, fp32 values around the overflow / underflow points of __expf (both signs) and values
    between the 16-bit grid points"""
    s = sweep16(dt, device).float()
    edges = torch.tensor(F32_EDGES, device=device)
    g = torch.Generator(device="cpu").manual_seed(5)
    rnd = (4 * torch.randn(4096, generator=g)).to(device)
    v = torch.cat([s, edges, -edges, rnd])
    return torch.cat([v, torch.zeros((-v.numel()) % 8, device=device)])


def softmax_rows_input(n, device):
    """the rows every softmax case runs, on the device and in the CPU emulation: random, constant, one key 80 above the
    rest, offset by -10000, spanning 120 units with the maximum in the LAST four-wide chunk, random again, and
    one key in the last chunk 100 above the rest (every other probability underflows)"""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(7, n, generator=g)
    x[1] = 0.75
    x[2, n // 2] += 80.0
    x[3] -= 10000.0
    x[4] = -120.0 * torch.rand(n, generator=g)
    x[4, n - 2] = 5.0
    x[5] *= 4.0
    x[6] -= 100.0
    x[6, n - 1] = 0.0
    return x.to(device)


# ---- bound class: references ------------------------------------------------------------------------------------------------
def _sig(a):
    return torch.sigmoid(a)


def act(kind, x):
    """x float64 (the exact inputs): (value, e) of one activation, e before any store"""
    ax = x.abs()
    if kind == "gelu":
        return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0)), GELU_ERF_ABS * ax.clamp_min(1.0)
    if kind == "silu":
        a = -x
    elif kind == "quick_gelu":
        a = -QUICK * x
    elif kind == "gelu_new":
        a = -2.0 * TANH_C0 * (x + TANH_C1 * x * x * x)
    else:
        raise ValueError(kind)
    v = x * _sig(-a)
    e = v.abs() * (ACT_REL + K_ARG[kind] * U32 * a.abs() * _sig(a)) + (ax + 1.0) * F32_TINY
    return v, e


def gated(kind, a, b):
    """out = act(a) * b: a, b float64"""
    v, e = act(kind, a)
    ref = v * b
    return ref, b.abs() * e + U32 * ref.abs()


def softmax_chain(n):
    return (n + 1023) // 1024 + 3 + 6 + 2


def softmax(x):
    """x fp32 [rows, n] -> (p, e) float64"""
    xd = x.double()
    d = xd - xd.amax(1, keepdim=True)
    E = d.exp()
    p = E / E.sum(1, keepdim=True)
    dE = 3 * U32 * d.abs() + EXP_REL
    rel = dE + (p * dE).sum(1, keepdim=True) + gamma(softmax_chain(x.shape[1])) + RCP + U32
    return p, 1.01 * p * rel


def timestep(t, n, dim, flip, freq_shift, scale, max_period):
    """t fp32 [t_count] -> (ref, e) float64 [n, dim] (row i: timestep t[i % t_count]); the float arguments as the C ABI passes them"""
    half = dim // 2
    j = torch.arange(half, dtype=torch.float64, device=t.device)
    ex = -math.log(fp32(max_period)) * j / (half - fp32(freq_shift))
    tt = t.double()[torch.arange(n, device=t.device) % t.numel()]
    arg = fp32(scale) * tt[:, None] * ex.exp()[None]
    e = arg.abs() * U32 * (K_ARG_T + K_EXP * ex.abs())[None] + SINCOS_ABS
    sn, cs = arg.sin(), arg.cos()
    parts = [cs, sn] if flip else [sn, cs]
    es = [e, e]
    if dim & 1:
        parts.append(torch.zeros(n, 1, dtype=torch.float64, device=t.device))
        es.append(torch.zeros(n, 1, dtype=torch.float64, device=t.device))
    return torch.cat(parts, 1), torch.cat(es, 1)


def axpby(x, y, coef):
    a, b = coef.double().tolist()
    ax, by = a * x.double(), b * y.double()
    return ax + by, 2 * U32 * (ax.abs() + by.abs())


def cfg_axpby(x, eu, et, coef, gs):
    a, b = coef.double().tolist()
    gs = fp32(gs)
    u, d = eu.double(), et.double() - eu.double()
    g = u + gs * d
    e_g = U32 * (3 * abs(gs) * d.abs() + u.abs())
    ax = a * x.double()
    return ax + b * g, abs(b) * e_g + 2 * U32 * (ax.abs() + abs(b) * (g.abs() + e_g))


def nchw(rows, B, L):
    """[B * HW, >= L] rows -> [B, L, HW]"""
    return rows[:, :L].reshape(B, -1, L).permute(0, 2, 1)


def latent_sample(m, B, L, noise, out_scale):
    """m fp32 rows [B * HW, >= 2 L], noise fp32 [B, L, HW] -> (ref, e) float64 [B, L, HW]"""
    s = fp32(out_scale)
    mu = nchw(m, B, L).double()
    lv = nchw(m[:, L:], B, L).double().clamp(-30.0, 20.0)
    sn = (0.5 * lv).exp() * noise.double()
    e = sn.abs() * (2 * U32 * (0.5 * lv).abs() + EXP_REL + U32) + 2 * U32 * (mu.abs() + sn.abs())
    return (mu + sn) * s, abs(s) * e


def check(out, ref, e):
    """worst |out - ref| / bound over every element of a 16-bit or fp32 output (non-finite -> inf; 0 / 0 passes). fp32: the kernels
    round once more after the value e bounds, so the bound is 2 * 2^-24 |ref| + e. The ratio alone: no rel-L2 is asked of these."""
    return BP.check(out, ref, e, f32_rel=2 * U32)[0]


# ---- exact class: plain torch restatements ------------------------------------------------------------------------------------
PATCH_AXES = ("b", "ty", "tx", "c", "py", "px")       # patchify: rows (b, ty, tx), columns (c, py, px)
UNPATCH_AXES = ("b", "c", "ty", "py", "tx", "px")     # unpatchify: NCHW with y = ty * p + py, x = tx * p + px


def patchify(x, p, dt, order=PATCH_AXES):
    """x fp32 [B, C, H, W] -> dt rows [B * (H / p) * (W / p), C * p * p]; `order` other than PATCH_AXES restates a FAULT"""
    B, C, H, W = x.shape
    src = {"b": 0, "c": 1, "ty": 2, "py": 3, "tx": 4, "px": 5}
    v = x.reshape(B, C, H // p, p, W // p, p).permute(*(src[a] for a in order))
    return v.reshape(B * (H // p) * (W // p), C * p * p).to(dt)


def unpatchify(x, B, C, H, W, p, cols=("py", "px", "c"), order=UNPATCH_AXES):
    """x 16-bit rows [B * h * w, p * p * C] with columns (py, px, c) -> fp32 [B, C, H, W]; other `cols` / `order`: a FAULT"""
    size = {"py": p, "px": p, "c": C}
    names = ("b", "ty", "tx") + tuple(cols)
    v = x.reshape(B, H // p, W // p, *(size[a] for a in cols))
    return v.permute(*(names.index(a) for a in order)).reshape(B, C, H, W).float()


def split_concat(x, y, order=("i", "c")):
    """x [B, S1, 3C], y [B, S2, 3C] -> (q, k, v) each [B, S1 + S2, C]; order ("c", "i") restates the interleaved-chunk FAULT"""
    B, _, H3 = x.shape
    C = H3 // 3
    z = torch.cat([x, y], 1)
    z = z.reshape(B, -1, 3, C) if order == ("i", "c") else z.reshape(B, -1, C, 3).transpose(2, 3)
    return tuple(z[:, :, i].contiguous() for i in range(3))


def embed_tokens(ids, tok, pos, seq_len):
    a = tok.float()[ids.long()]
    b = pos.float()[torch.arange(ids.numel(), device=ids.device) % seq_len] if pos is not None else 0.0
    return (a + b).to(tok.dtype)


def add_nchw(x, r, order=(0, 2, 1)):
    """x [B, HW, C] (16-bit or fp32) += r fp32 [B, C, HW]"""
    return (x.float() + r.permute(*order).reshape(x.shape)).to(x.dtype)


def mask_to_bias(mask):
    return (1.0 - mask) * -10000.0


def latent_moments(m, B, L, out_scale):
    """(mean, clipped logvar, the noise == NULL sample) fp32 [B, L, HW]"""
    mu = nchw(m, B, L).contiguous()
    lv = nchw(m[:, L:], B, L).clamp(-30.0, 20.0).contiguous()
    return mu, lv, (mu + 0.0) * torch.tensor(out_scale, dtype=torch.float32, device=m.device)   # (-0 + 0 = +0, as the kernel)
