"""Attention inputs on which the float64 bound of tests/attn_bounds.py is sharp: shared by the CPU proof (tests/test_attn_bounds.py,
scaled-down shapes against an emulation of the flash loop) and the GPU matrix (tests/attn_child.py, every kernel form).

Kinds:
  S1  uniform keys: within each (b, h) every key row is the same (a different row per (b, h)); q, v random; exact_p. The answer is
      the mean of the valid v rows: a dropped or repeated tile, a wrong (b, h) base or phantom tail keys move it far past the bound
      (one phantom key moves the mean by ~1 / (Skv + 1): the tail cases keep Skv short).
  S2  one-hot selectors: q_i = fl(alpha_i k_pi(i)) with a float64-checked margin of MARGIN nats over every other key of the row;
      pi hits key 0, keys 63 / 64 (either side of a tile boundary), the first and last valid key of a ragged tail, and random keys.
      Every query row, those of the partial last query block included, selects one. The answer is v_pi(i).
  S2g the same above the lazy guard's range (MARGIN_GUARD nats: > 60 log2 units, LAZY_PSUM_LIMIT of the bf16 build), with the
      selected keys late in the row: the lazy kernels redo those tiles the exact way, the others rescale.
  S2b bias selector: small random q, k, bias; +60 on key pi(i) in the bias. Pins the bias addressing of every layout.
  S3  Skv = 1: out == v bit for bit.
  S4  random inputs (today's cases): under the bound, and rel-L2 against float64 below the suite's bar.

Bias layouts: b11k [B, 1, 1, Skv] (the encoder mask), 1hqk [1, H, Sq, Skv] (T5's relative-position bias, batch stride 0), bhqk
[B, H, Sq, Skv], keep (b11k of 0 / -10000: the UNet's keep-mask), unet (keep with scale = ln 2 and q carrying D^-0.5 log2(e): the
UNet builder's masked log2 form, unet.py attention()).
"""
import math

import torch

MARGIN = 40.0
MARGIN_GUARD = 50.0
LOG2E = 1.4426950408889634


def tail_keys(Skv):
    """the selected keys S2 must hit"""
    ks = {0, 63, 64, Skv - 1, (Skv // 64) * 64}
    return sorted(j for j in ks if 0 <= j < Skv)


def _mask_rows(shape, gen, device):
    """0 / -10000 keep-mask with ~1/4 of the keys masked, key 0 never (so no row is empty)"""
    m = torch.rand(shape, generator=gen, device=device) < 0.25
    m[..., 0] = False
    return torch.where(m, torch.full(shape, -10000.0, device=device), torch.zeros(shape, device=device))


def _bias_shape(layout, B, H, Sq, Skv):
    return {"b11k": (B, 1, 1, Skv), "keep": (B, 1, 1, Skv), "unet": (B, 1, 1, Skv), "1hqk": (1, H, Sq, Skv),
            "bhqk": (B, H, Sq, Skv)}[layout]


def make(spec, dt, device="cpu", seed=0):
    """inputs of one case: dict(q, k, v, bias, scale, log2, accum, old, exact_p). spec: dict(B, H, Sq, Skv, D, kind, bias=None,
    log2=False, accum=None)."""
    B, H, Sq, Skv, D = (spec[n] for n in ("B", "H", "Sq", "Skv", "D"))
    kind, layout, log2 = spec["kind"], spec.get("bias"), spec.get("log2", False)
    gen = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, device=device)   # noqa: E731
    scale = math.log(2.0) if layout == "unet" else 1.0 / math.sqrt(D)
    sc = math.log(2.0) if log2 else scale                 # natural units per unit of q.k
    qmul = D ** -0.5 * LOG2E if (log2 or layout == "unet") else 1.0
    v = rn(B, Skv, H, D).to(dt)
    bias = None
    exact_p = False
    if layout is not None:
        shp = _bias_shape(layout, B, H, Sq, Skv)
        if layout in ("keep", "unet") or kind == "S1":
            bias = _mask_rows(shp, gen, device)
        elif kind == "S2b":
            bias = 0.5 * rn(*shp)
        else:
            bias = rn(*shp) * (0.5 if kind == "S2" else 1.0)
    if kind == "S1":
        k = rn(B, 1, H, D).expand(B, Skv, H, D).contiguous().to(dt)
        q = (rn(B, Sq, H, D) * qmul).to(dt)
        exact_p = True
    elif kind in ("S2", "S2g"):
        k = rn(B, Skv, H, D)
        k = (k / k.norm(dim=-1, keepdim=True)).to(dt)
        q = _selectors(k, bias, B, H, Sq, Skv, D, sc, gen, device, dt, MARGIN_GUARD if kind == "S2g" else MARGIN, late=kind == "S2g")
    elif kind == "S2b":
        k = (0.3 * rn(B, Skv, H, D)).to(dt)
        q = (0.3 * rn(B, Sq, H, D) * qmul).to(dt)
        pi = _pick(Sq, Skv, gen, device, n=bias.shape[2] if bias.shape[2] > 1 else 1)   # [Sq | 1]
        bias[..., torch.arange(pi.numel(), device=device), pi] += 60.0
    elif kind in ("S3", "S4"):
        assert kind != "S3" or Skv == 1
        k = rn(B, Skv, H, D).to(dt)
        q = (rn(B, Sq, H, D) * qmul).to(dt)
    else:
        raise ValueError(kind)
    accum = spec.get("accum")
    old = rn(B, Sq, H, D).to(dt) if accum is not None else None
    return dict(q=q, k=k, v=v, bias=bias.contiguous() if bias is not None else None, scale=scale, log2=log2, accum=accum, old=old,
                exact_p=exact_p)


def _pick(Sq, Skv, gen, device, n=None, late=False):
    """selected key per query row: the tail_keys() in turn, every third row a random key (late: keys from the second tile on)"""
    n = Sq if n is None else n
    fixed = torch.tensor([j for j in tail_keys(Skv) if not late or j >= 64] or [Skv - 1], device=device)
    lo = 64 if late and Skv > 64 else 0
    rnd = torch.randint(lo, Skv, (n,), generator=gen, device=device)
    i = torch.arange(n, device=device)
    return torch.where(i % 3 == 2, rnd, fixed[i % fixed.numel()])


def _selectors(k, bias, B, H, Sq, Skv, D, sc, gen, device, dt, margin, late):
    """q rows that each select one key by `margin` nats (float64-checked on the rounded q, bias included)"""
    q = torch.empty(B, Sq, H, D, device=device)
    for b in range(B):
        for h in range(H):
            K = k[b, :, h].double()
            pi = _pick(Sq, Skv, gen, device, late=late)
            kp = K[pi]                                        # [Sq, D]
            bb = None
            if bias is not None:
                bb = bias[b if bias.shape[0] > 1 else 0, h if bias.shape[1] > 1 else 0].double().expand(Sq, Skv)
            alpha = torch.full((Sq, 1), 2.0 * margin / sc, dtype=torch.float64, device=device)
            rows = torch.arange(Sq, device=device)
            for _ in range(40):
                qq = (alpha * kp).to(dt)
                x = sc * (qq.double() @ K.t())
                if bb is not None:
                    x = x + bb
                xp = x[rows, pi].clone()
                x[rows, pi] = -math.inf
                short = (xp - x.amax(1)) < margin
                if not short.any():
                    break
                alpha[short] *= 1.5
            else:
                raise AssertionError("selector margin not reached")
            q[b, :, h] = qq.float()
    return q.to(dt)
