"""The fused step-tail entries of include/mi355x_sd.h (csrc/step_tail.hip), one row each: the argument contract of
mi355x_sd_<entry>(<operands>, guidance_scale, guidance_rescale, batch, per_sample, stream)  and what the denoising loop needs to call
it. The ctypes signatures (_lib.py), the wrappers' checks (ops.py), the loop's tails (pipeline.py) and the tests' emulators and
refusal tables (tests/step_forms.py) are all read from here; tests/test_step_forms.py holds every row to the header's declaration,
and the C entry (csrc/capi.hip step_entry) states the same row once more, in C.

An operand is a pointer to batch * per_sample floats unless the row says otherwise:
  operands       in the header's order, under the header's parameter names; ``order`` is the one int among them
  width, align   ``coef`` is `width` floats at a multiple of `align` bytes
  written        {operand: planes} of every span the launch writes (None: as many planes as ``order``)
  optional       the pointers that may be null
  same           the (written, read) pairs that may be one pointer
  always_rescale the guidance rescale runs whatever guidance_rescale is (per_sample >= 2 always; eps_text is needed)
  coef_overlaps  ``coef`` takes part in the overlap rule
and for the loop (paddlemix_amd/pipeline.py _FusedTail):
  walk           the scheduler method that gives a step's coefficient row
  whole_schedule a stateless row, walked over the scheduler's WHOLE schedule with its model-input scale: row i. False: a row depends
                 on the steps before it, the walk covers the timesteps the loop RUNS: row i - first
  state          {operand: planes} of the buffers the tail owns for the whole loop (None: ``order`` planes); a written operand that is
                 not listed is the `same` partner that is
  noise          None; "fresh": a new ``torch.randn`` plane per step; "reused": drawn into one buffer (``out=``) when the scheduler's
                 ``step`` takes a generator, a null pointer when it does not"""
from collections import namedtuple

StepForm = namedtuple("StepForm", "entry operands width align written optional same always_rescale coef_overlaps walk whole_schedule "
                                  "state noise")
TAIL = ("guidance_scale", "guidance_rescale", "batch", "per_sample")   # what follows the operands in every signature (then the stream)


def _form(entry, operands, width, written, walk, state, *, optional=("eps_text",), same=(("out", "x"),), align=1, whole_schedule=False,
          noise=None, always_rescale=False, coef_overlaps=True):
    return StepForm(entry, tuple(operands.split()), width, align, written, optional, same, always_rescale, coef_overlaps, walk,
                    whole_schedule, state, noise)


FORMS = {
    "guidance": _form("cfg_rescale_axpby", "x eps_uncond eps_text out coef", 2, {"out": 1}, "step_coefficients", {}, optional=(),
                      whole_schedule=True, always_rescale=True, coef_overlaps=False),
    "multistep": _form("multistep_update", "x eps_uncond eps_text m_prev out m_out coef", 5, {"out": 1, "m_out": 1},
                       "multistep_coefficients", {"m_prev": 1}, same=(("out", "x"), ("m_out", "m_prev"))),
    "unipc": _form("unipc_update", "x eps_uncond eps_text last hist order out coef", 12, {"out": 1, "last": 1, "hist": None},
                   "unipc_coefficients", {"last": 1, "hist": None}, align=16),
    "ancestral": _form("ancestral_update", "x eps_uncond eps_text noise out coef", 3, {"out": 1}, "ancestral_coefficients", {},
                       optional=("eps_text", "noise"), whole_schedule=True, noise="fresh"),
    "heun": _form("heun_update", "x eps_uncond eps_text sample deriv out coef", 5, {"out": 1, "sample": 1, "deriv": 1},
                  "heun_coefficients", {"sample": 1, "deriv": 1}, whole_schedule=True),
    "dpm2": _form("dpm2_update", "x eps_uncond eps_text noise sample out coef", 5, {"out": 1, "sample": 1}, "dpm2_coefficients",
                  {"sample": 1}, optional=("eps_text", "noise"), whole_schedule=True, noise="reused"),
    "plms": _form("plms_update", "x eps_uncond eps_text park hist out coef", 12, {"out": 1, "park": 1, "hist": 3}, "plms_coefficients",
                  {"park": 1, "hist": 3}),
    "singlestep": _form("singlestep_update", "x eps_uncond eps_text park hist out coef", 8, {"out": 1, "park": 1, "hist": 2},
                        "singlestep_coefficients", {"park": 1, "hist": 2}),
}


def signature(form):
    """(restype, argtypes) of the row's entry for _lib.SIGNATURES"""
    from ctypes import c_float, c_int, c_int64, c_void_p
    return c_int, [c_int if k == "order" else c_void_p for k in form.operands] + [c_float, c_float, c_int, c_int64, c_void_p]
