"""The cases of the panorama tests (tests/test_panorama_host.py, tests/panorama_child.py, tests/test_gpu_panorama.py,
scripts/make_panorama_golden.py) -- TEST INFRASTRUCTURE ONLY: the kernel matrix of mi355x_sd_view_input / mi355x_sd_view_merge, their
inputs, and the settings of the recorded loops. The stand-in U-Net is tests/sega_cases.py's FormulaUNet."""
import torch

from paddlemix_amd import schedulers as S
from tests.sega_cases import SCHED, SCHEDULERS as _SEGA_SCHEDULERS, FormulaUNet   # noqa: F401

GS = 7.5
SCHEDULERS = dict(_SEGA_SCHEDULERS, pndm=lambda: S.PNDMScheduler(skip_prk_steps=True, steps_offset=1, **SCHED))


# ------------------------------------------------------------------------------------------------- the kernel matrix
# Both kernels have two paths: 16-byte vectors (W, win_w, stride multiples of 4, aligned pointers) and element by element. The
# geometries: a plain row of views; columns no view covers (8 x 22); a wrap (circular); two rows of views (counts up to 4); a window
# and stride no vector fits, with the wrap inside what would be one (6 / 3 on 15 columns); stride 1 (up to 8 views per column: the
# divisors 3, 5, 6, 7); the pipeline's own 64 / 8; a window clipped to a source lower than it (5 rows); a middle chunk of views; every
# pointer 4 bytes off. Each at batch 1 and 2; the input at 1 and 2 groups.
def _geo(H, W, win_h, win_w, stride, circular=False, C=3, first=None, count=None, off=0):
    ny = (H - win_h) // stride + 1
    nx = W // stride if circular and W > win_w else (W - win_w) // stride + 1
    return dict(H=H, W=W, win_h=win_h, win_w=win_w, stride=stride, ny=ny, nx=nx, circular=int(circular), C=C, first=first, count=count, off=off)


GEOMETRIES = {
    "w8s4 8x20": _geo(8, 20, 8, 8, 4),
    "w8s4 8x22 uncovered": _geo(8, 22, 8, 8, 4),
    "w8s4 8x20 circular": _geo(8, 20, 8, 8, 4, True),
    "w8s4 12x20 two rows": _geo(12, 20, 8, 8, 4),
    "w6s3 6x15": _geo(6, 15, 6, 6, 3),
    "w6s3 6x15 circular": _geo(6, 15, 6, 6, 3, True),
    "w8s1 8x16": _geo(8, 16, 8, 8, 1),
    "w64s8 64x80": _geo(64, 80, 64, 64, 8, C=4),
    "w64s8 64x80 circular": _geo(64, 80, 64, 64, 8, True, C=4),
    "w5x8s4 5x20 clipped": _geo(5, 20, 5, 8, 4),
    "w64s8 64x80 circular views 3..6": _geo(64, 80, 64, 64, 8, True, C=4, first=3, count=4),
    "w8s4 12x20 two rows views 2..4": _geo(12, 20, 8, 8, 4, first=2, count=3),
    "w8s4 8x20 circular off4": _geo(8, 20, 8, 8, 4, True, off=1),
    "w64s8 64x80 off4": _geo(64, 80, 64, 64, 8, C=4, off=1),
}
KERNEL = {f"{name} b{b}": dict(g, batch=b) for name, g in GEOMETRIES.items() for b in (1, 2)}
SCALE = 0.7071067690849304   # an fp32 value with a full mantissa: x * SCALE rounds on almost every element


def vector_path(spec):
    """csrc/panorama.hip view_vec: the alignment rule of both kernels"""
    return int(spec["off"] == 0 and spec["W"] % 4 == 0 and spec["win_w"] % 4 == 0 and spec["stride"] % 4 == 0)


def cover(spec):
    """[ny * nx, H, W] bool: the elements view v covers"""
    out = torch.zeros(spec["ny"] * spec["nx"], spec["H"], spec["W"], dtype=torch.bool)
    for v in range(spec["ny"] * spec["nx"]):
        iy, ix = divmod(v, spec["nx"])
        cols = torch.arange(spec["win_w"]) + ix * spec["stride"]
        out[v, iy * spec["stride"]:iy * spec["stride"] + spec["win_h"], cols % spec["W"] if spec["circular"] else cols] = True
    return out


def kernel_inputs(spec, seed):
    """-> (x [B, C, H, W], views [ny * nx * B, C, win_h, win_w]): fp32 CPU normal draws; channel 1 carries a common offset of 50;
    planted in image 0, channel 0: -0.0 at an element of x and, in the views, at EVERY view element that lands on output element
    (0, 1) (the merge must give +0.0 there), +inf, -inf and one NaN at three other places"""
    B, C, H, W, wh, ww = spec["batch"], spec["C"], spec["H"], spec["W"], spec["win_h"], spec["win_w"]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    views = torch.randn(spec["ny"] * spec["nx"] * B, C, wh, ww, generator=g)
    x[:, 1] += 50.0
    views[:, 1] += 50.0
    x[0, 0, 0, 1], x[0, 0, 1, 2], x[0, 0, 2, 3], x[0, 0, 3, 0] = -0.0, float("inf"), float("-inf"), float("nan")
    for v in range(spec["ny"] * spec["nx"]):
        iy, ix = divmod(v, spec["nx"])
        j = (1 - ix * spec["stride"]) % W if spec["circular"] else 1 - ix * spec["stride"]
        if iy == 0 and 0 <= j < ww:
            views[v * B, 0, 0, j] = -0.0
    views[0, 0, 1, 2], views[0, 0, 2, 3], views[0, 0, 3, 0] = float("inf"), float("-inf"), float("nan")
    return x, views


# ------------------------------------------------------------------------------------------------- the loops
STEPS, TOKENS, DIM = 4, 7, 32
GOLDEN_SEED = 41
SHAPES = {   # name: (latent shape, circular_padding, view_batch_size): 3 views; 10 views, the last chunk short; 2 x 2 views, 4 uncovered columns
    "plain": ((1, 4, 64, 80), False, 1),
    "circular": ((1, 4, 64, 80), True, 3),
    "two_rows": ((2, 4, 72, 76), False, 2),
}
GOLDEN = {   # name: (scheduler, shape, guidance_scale)
    "ddim_plain": ("ddim", "plain", GS),
    "heun_plain": ("heun", "plain", GS),
    "euler_circular": ("euler", "circular", GS),
    "dpm_circular": ("dpm", "circular", GS),
    "pndm_two_rows": ("pndm", "two_rows", GS),
    "ddim_two_rows_unguided": ("ddim", "two_rows", 1.0),
}


def loop_inputs(shape):
    """(prompt_embeds [B, T, D], negative [B, T, D], initial noise): ONE prompt repeated over the batch, where the reference's pairing
    of images and prompts agrees with this project's"""
    g = torch.Generator().manual_seed(GOLDEN_SEED)
    pe, ne = torch.randn(1, TOKENS, DIM, generator=g), torch.randn(1, TOKENS, DIM, generator=g) - 0.2
    lat = torch.randn(*shape, generator=g)
    return pe.repeat(shape[0], 1, 1), ne.repeat(shape[0], 1, 1), lat
