"""The two InstructPix2Pix entries of include/mi355x_sd.h (csrc/ip2p.hip, ABI 24), one row each: the argument contract of
mi355x_sd_<entry>. The ctypes signatures (_lib.py) and the tests' emulator and refusal table (tests/abi_emulator_ip2p.py,
tests/test_ip2p_host.py) are read from here; the tensor-level wrappers (ops.guidance3, ops.ip2p_input) state their own shape checks; the C entries (csrc/capi.hip span_entry) state the same
rows once more, in C, and tests/test_ip2p_host.py holds every row to the header's declaration.

  params    (C type, name) in the header's order, the stream last
  spans     {pointer: floats it spans}, a function of the call's arguments by name
  written   the pointers the launch writes: such a span overlaps no other span
  optional  the pointers that may be null where they are used
  positive  the integers that must be >= 1
  used      pointer -> a predicate of the arguments: the operand takes part in the call (and in the null and overlap rules) only
            when it holds"""
from collections import namedtuple

Entry = namedtuple("Entry", "entry params spans written optional positive used")

_rescaled = lambda a: a["guidance_rescale"] > 0.0   # noqa: E731

ENTRIES = {
    "guidance3": Entry(
        "guidance3",
        (("const float*", "eps"), ("const float*", "x"), ("const float*", "coef"), ("float*", "out"), ("float", "guidance_scale"),
         ("float", "image_guidance_scale"), ("float", "guidance_rescale"), ("int", "batch"), ("int64_t", "per_sample"), ("void*", "stream")),
        {"eps": lambda a: 3 * a["batch"] * a["per_sample"], "x": lambda a: a["batch"] * a["per_sample"], "coef": lambda a: 1,
         "out": lambda a: a["batch"] * a["per_sample"]},
        ("out",), ("x",), ("batch", "per_sample"),
        {"x": _rescaled, "coef": lambda a: _rescaled(a) and bool(a["x"])}),
    "ip2p_input": Entry(
        "ip2p_input",
        (("const float*", "x"), ("const float*", "image_latents"), ("float*", "out"), ("float", "scale"), ("int", "groups"), ("int", "batch"),
         ("int", "c_lat"), ("int", "c_img"), ("int64_t", "hw"), ("void*", "stream")),
        {"x": lambda a: a["batch"] * a["c_lat"] * a["hw"], "image_latents": lambda a: a["groups"] * a["batch"] * a["c_img"] * a["hw"],
         "out": lambda a: a["groups"] * a["batch"] * (a["c_lat"] + a["c_img"]) * a["hw"]},
        ("out",), (), ("groups", "batch", "c_lat", "c_img", "hw"), {}),
}


def signature(entry):
    """(restype, argtypes) of the row's entry for _lib.SIGNATURES"""
    from ctypes import c_float, c_int, c_int64, c_void_p
    by_value = {"int": c_int, "int64_t": c_int64, "float": c_float}
    return c_int, [by_value.get(kind, c_void_p) for kind, _ in entry.params]
