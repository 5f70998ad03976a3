"""Panorama / MultiDiffusion (csrc/panorama.hip, ABI 26): the argument contracts of mi355x_sd_view_input and mi355x_sd_view_merge as
rows of the type ip2p_forms.Entry (the ctypes signatures, the tests' emulator and refusal table are read from them), the view
geometry the two kernels and the loop share, and its range rule -- csrc/capi.hip view_rule states the same rules in the same order.

The geometry is the reference's ``get_views`` (pipeline_stable_diffusion_panorama.py:473-491) in latent units, window and stride as
arguments: ny x nx views, view v = iy * nx + ix at row iy * stride, column ix * stride, win_h x win_w elements; with ``circular``
column j of a view is source column (ix * stride + j) mod W. Rows never wrap."""
from .ip2p_forms import Entry

WINDOW, STRIDE = 64, 8      # the reference's window_size and stride (its get_views defaults; the pipeline passes no others)
CIRCULAR_PAD = 8            # decode_latents_with_padding's `padding`, in latent columns (:371)
INT64_MAX = 2 ** 63 - 1
MAX_PLANES = 65535          # csrc/panorama.hip: grid.z holds (sample, channel)

_GEOMETRY = (("int", "batch"), ("int", "C"), ("int", "H"), ("int", "W"), ("int", "win_h"), ("int", "win_w"), ("int", "stride"),
             ("int", "ny"), ("int", "nx"), ("int", "circular"))
_window = lambda a: a["batch"] * a["C"] * a["win_h"] * a["win_w"]   # noqa: E731
_source = lambda a: a["batch"] * a["C"] * a["H"] * a["W"]   # noqa: E731
_DIMS = ("batch", "C", "H", "W", "win_h", "win_w", "stride", "ny", "nx")

ENTRIES = {
    "view_input": Entry(
        "view_input",
        (("const float*", "x"), ("float*", "out"), ("float", "scale"), ("int", "groups")) + _GEOMETRY +
        (("int", "first"), ("int", "count"), ("void*", "stream")),
        {"x": _source, "out": lambda a: a["groups"] * a["count"] * _window(a)}, ("out",), (), _DIMS, {}),
    "view_merge": Entry(
        "view_merge", (("const float*", "views"), ("float*", "out")) + _GEOMETRY + (("void*", "stream"),),
        {"views": lambda a: a["ny"] * a["nx"] * _window(a), "out": _source}, ("out",), (), _DIMS, {}),
}


def grid(h, w, window=WINDOW, stride=STRIDE, circular=False):
    """(ny, nx, win_h, win_w) of a [.., h, w] latent: ``get_views``' block counts, the window clipped to the latent on an axis it
    exceeds (what the reference's slicing does to a window that leaves the tensor)"""
    ny = (h - window) // stride + 1 if h > window else 1
    if circular:
        nx = w // stride if w > window else 1
    else:
        nx = (w - window) // stride + 1 if w > window else 1
    return ny, nx, min(window, h), min(window, w)


def views(h, w, window=WINDOW, stride=STRIDE, circular=False):
    """[(h_start, h_end, w_start, w_end)] in view order, as ``get_views`` lists them (the ends unclipped, as there)"""
    ny, nx, _, _ = grid(h, w, window, stride, circular)
    return [(iy * stride, iy * stride + window, ix * stride, ix * stride + window) for iy in range(ny) for ix in range(nx)]


def geometry_rule(a):
    """the name of the first geometry rule the arguments `a` (by name) break, or None: csrc/capi.hip view_rule"""
    for k in _DIMS:
        if a[k] < 1:
            return k
    if a["win_h"] > a["H"]:
        return "win_h"
    if a["win_w"] > a["W"]:
        return "win_w"
    if (a["ny"] - 1) * a["stride"] + a["win_h"] > a["H"]:
        return "ny"
    if not a["circular"] and (a["nx"] - 1) * a["stride"] + a["win_w"] > a["W"]:
        return "nx"
    if a["circular"] and (a["nx"] - 1) * a["stride"] >= a["W"]:
        return "nx"
    if 4 * _source(a) > INT64_MAX:
        return "H, W"
    if 4 * a["ny"] * a["nx"] * _window(a) > INT64_MAX:
        return "ny, nx"
    return None
