"""Semantic guidance (SEGA; csrc/sega.hip, ABI 25): the argument contract of mi355x_sd_sega_guidance as one row of the type
ip2p_forms.Entry (the ctypes signature, the tests' emulator and refusal table are read from it), and the per-step table the kernel
reads its scalars from.

The table. Everything the reference decides per step on the host (pipeline_semantic_stable_diffusion.py:581-613, :653-691: the
scalar-or-list arguments, warm-up, cool-down, the regime, the concept weights and their normalisation, the rank of the quantile) is
decided here once per call, for every step, and uploaded as ``[steps][ROW_HEAD + ROW_PER * n]`` 32-bit words; a step passes its row's
address, so a captured step replays with the next row. A row:

  word 0  regime      int    0 none warm, 1 partial (0 < |warm| < n, :654-677), 2 all warm (:691)
  word 1  active      int    bit c: concept c is not cooled down (i < cooldown_c); a cleared bit is g_c = 0 and weight 0 (:611-613)
  word 2  warm        int    bit c: i >= warmup_c
  word 3  (unused)
  word 4  gs          fp32   guidance_scale
  word 5  ms          fp32   edit_momentum_scale
  word 6  beta        fp32   edit_mom_beta
  word 7  omb         fp32   1 - edit_mom_beta, rounded from the float64 difference as a Python scalar times a tensor is
  then per concept c, ROW_PER words at ROW_HEAD + ROW_PER * c:
  +0  scale   fp32   +-edit_guidance_scale_c (minus: reverse_editing_direction_c)
  +1  lo      int    floor(rank), rank = fp32(threshold_c) * fp32(hw - 1) in fp32: torch.quantile's rule
  +2  frac    fp32   rank - lo (exact); 0 means hi = lo, otherwise hi = lo + 1
  +3  w_full  fp32   nan_to_num(max(w_c, 0)), w_c = edit_weights[c] or 1, 0 when cooled down (:679-685)
  +4  w_part  fp32   max(w_c, 0) / sum over warm of max(w, 0) (no nan_to_num: a zero sum is NaN, :659-662); 0 outside warm"""
import numpy as np

from .ip2p_forms import Entry

MAX_CONCEPTS = 8      # csrc/sega.hip SEGA_MAX_CONCEPTS: the bits of `active` / `warm` a row carries, the kernel's register arrays
MAX_HW = 65536        # csrc/sega.hip SEGA_MAX_HW: a 256 x 256 latent
ROW_HEAD, ROW_PER = 8, 5
REGIME_NONE, REGIME_PARTIAL, REGIME_ALL = 0, 1, 2

_planes = lambda a: a["batch"] * a["channels"] * a["hw"]   # noqa: E731

ENTRIES = {
    "sega_guidance": Entry(
        "sega_guidance",
        (("const float*", "eps"), ("float*", "momentum"), ("const float*", "extra"), ("const float*", "row"), ("float*", "out"),
         ("float*", "stats"), ("int", "n_concepts"), ("int", "batch"), ("int", "channels"), ("int64_t", "hw"), ("void*", "stream")),
        {"eps": lambda a: (2 + a["n_concepts"]) * _planes(a), "momentum": _planes, "extra": _planes,
         "row": lambda a: ROW_HEAD + ROW_PER * a["n_concepts"], "out": _planes,
         "stats": lambda a: 3 * a["n_concepts"] * a["batch"] * a["channels"]},
        ("momentum", "out", "stats"), ("extra", "stats"), ("n_concepts", "batch", "channels", "hw"),
        {"extra": lambda a: bool(a["extra"]), "stats": lambda a: bool(a["stats"])}),
}


def row_words(n):
    return ROW_HEAD + ROW_PER * n


def per_concept(value, c):
    """the reference's scalar-or-list rule (:581-608): a list is indexed by the concept, anything else serves every concept"""
    return value[c] if isinstance(value, list) else value


def quantile_rank(q, hw):
    """(lo, frac) of torch.quantile's linear interpolation over hw values: rank = q * (hw - 1) in fp32"""
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"`edit_threshold` must be in the range [0, 1], got {q}")
    rank = np.float32(q) * np.float32(hw - 1)
    lo = np.floor(rank)
    return int(lo), np.float32(rank - lo)


def step_decisions(i, n, reverse_editing_direction=False, edit_guidance_scale=5, edit_warmup_steps=10, edit_cooldown_steps=None,
                   edit_threshold=0.9, edit_weights=None):
    """the reference's decisions at step i, per concept: (scale, threshold, weight or None when cooled down, warm)"""
    out = []
    for c in range(n):
        scale = np.float32(per_concept(edit_guidance_scale, c))
        if per_concept(reverse_editing_direction, c):
            scale = -scale
        cooldown = per_concept(edit_cooldown_steps, c) if isinstance(edit_cooldown_steps, list) else \
            (i + 1 if edit_cooldown_steps is None else edit_cooldown_steps)
        weight = np.float32(edit_weights[c] if edit_weights else 1.0)
        out.append((scale, float(per_concept(edit_threshold, c)), None if i >= cooldown else weight,
                    i >= per_concept(edit_warmup_steps, c)))
    return out


def rows(steps, n, hw, guidance_scale, edit_momentum_scale=0.1, edit_mom_beta=0.4, **per_concept_args):
    """-> uint32 [steps, row_words(n)]: row i is step i's (the loop's i: a scheduler of order 2 runs more steps than it was asked)"""
    if not 1 <= n <= MAX_CONCEPTS:
        raise NotImplementedError(f"semantic guidance takes 1 .. {MAX_CONCEPTS} editing prompts, got {n}")
    if not 1 <= hw <= MAX_HW:
        raise NotImplementedError(f"semantic guidance takes latent planes of up to {MAX_HW} elements, got {hw}")
    table = np.zeros((steps, row_words(n)), dtype=np.uint32)
    f = table.view(np.float32)
    zero = np.float32(0.0)
    with np.errstate(all="ignore"):
        for i in range(steps):
            dec = step_decisions(i, n, **per_concept_args)
            warm = [c for c, d in enumerate(dec) if d[3]]
            clamped = [zero if d[2] is None else (zero if d[2] < 0 else d[2]) for d in dec]   # where(w < 0, 0, w): a NaN stays
            total = zero
            for c in warm:
                total = np.float32(total + clamped[c])
            table[i, 0] = REGIME_ALL if len(warm) == n else (REGIME_PARTIAL if warm else REGIME_NONE)
            table[i, 1] = sum(1 << c for c, d in enumerate(dec) if d[2] is not None)
            table[i, 2] = sum(1 << c for c in warm)
            f[i, 4], f[i, 5], f[i, 6] = guidance_scale, edit_momentum_scale, edit_mom_beta
            f[i, 7] = 1 - edit_mom_beta
            for c, (scale, q, _, _) in enumerate(dec):
                at = ROW_HEAD + ROW_PER * c
                lo, frac = quantile_rank(q, hw)
                f[i, at], table[i, at + 1], f[i, at + 2] = scale, lo, frac
                f[i, at + 3] = np.nan_to_num(clamped[c])
                f[i, at + 4] = np.float32(clamped[c] / total) if c in warm else zero
    return table
