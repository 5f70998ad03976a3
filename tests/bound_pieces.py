"""What the kernel families' bound modules (tests/*_bounds.py) share: the constants of the output rounding, the comparison of an
output against a float64 reference and its elementwise error, and the bit-exact comparison. Plain Python + torch; runs on whatever
device the tensors live on. A family keeps what carries its knowledge -- the derivation, reference(), its own constants -- and its
check() is one call of check() here, with the family's conventions passed as named arguments.

16-bit store: |out - ref| <= u_out |ref| + (1 + u_out) e + 2^-24, u_out twice the unit roundoff of the element type (a correct
kernel sits at or below half of the bound; the last term is fp16's subnormal spacing). An explicit u_out takes the same form.
fp32 store: |out - ref| <= f32_rel |ref| + e with no floor, so an element with err = bound = 0 passes. f32_rel is the family's:
2^-24 where the stored value is the epilogue value itself (the GEMMs, the convolutions), 2 * 2^-24 where the kernel rounds once more
(the row-map kernels).
rel-L2: |out - ref| / max(|ref|, rel_floor). rel_floor = 0 leaves the denominator as it is (a zero reference gives NaN or inf)."""
import torch

U32 = 2.0 ** -24
U_OUT = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}


def fp32(x: float) -> float:
    """the value a float argument of the C ABI arrives with"""
    return float(torch.tensor(x, dtype=torch.float32))


def check(out, ref, e, *, u_out=None, f32_rel=None, rel_floor=0.0):
    """(worst |out - ref| / bound over every element, rel-L2) of `out` against a float64 (ref, e); a non-finite output or a NaN
    ratio -> inf. An fp32 `out` without an explicit u_out takes the fp32 form and needs f32_rel."""
    o = out.double()
    err = (o - ref).abs()
    if out.dtype == torch.float32 and u_out is None:
        bound = f32_rel * ref.abs() + e
        bound = torch.where((bound == 0) & (err == 0), torch.ones_like(bound), bound)   # (an exact zero: 0 / 0 is a pass)
    else:
        u = U_OUT[out.dtype] if u_out is None else u_out
        bound = u * ref.abs() + (1 + u) * e + U32
    ratio = (err / bound).max().item()
    if not torch.isfinite(o).all() or ratio != ratio:
        ratio = float("inf")
    rel = ((o - ref).norm() / ref.norm().clamp_min(rel_floor)).item()
    return ratio, rel


def exact_off(a, b):
    """number of elements whose bits differ, over 1-, 2- and 4-byte elements (a shape or dtype mismatch: every element)"""
    if tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype:
        return max(a.numel(), b.numel())
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.element_size()]
    return int((a.contiguous().view(it) != b.contiguous().view(it)).sum().item())
