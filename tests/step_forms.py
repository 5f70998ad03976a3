"""The seven fused step-tail entries of include/mi355x_sd.h as the tests see them -- TEST INFRASTRUCTURE ONLY: one row per form, read
by the emulators' argument rule (tests/abi_emulator_guidance.py step_args), the GPU children's harness (tests/step_child.py) and the
loop tests' recorder (tests/step_pieces.py). tests/test_step_forms.py holds every row to its signature in paddlemix_amd/_lib.py.

Every entry is  mi355x_sd_<entry>(<operands>, gs, gr, batch, per_sample, stream)  and ops.<entry> is its wrapper. An operand is a
pointer to batch * per_sample floats unless the row says otherwise: `written` gives the planes of each span the launch writes (None:
as many as the int operand `order`), `coef` is `width` floats, `optional` names the pointers that may be null, `same` the
(written, read) pairs that may be one pointer."""
from collections import namedtuple

Form = namedtuple("Form", "entry operands width written optional same")
TAIL = ("gs", "gr", "batch", "n")   # what follows the operands in every signature (then the stream)


def _form(entry, operands, width, written, optional=("et",), same=(("out", "x"),)):
    return Form(entry, tuple(operands.split()), width, written, optional, same)


FORMS = {
    "guidance": _form("cfg_rescale_axpby", "x eu et out coef", 2, {"out": 1}, optional=()),
    "multistep": _form("multistep_update", "x eu et m1 out m_out coef", 5, {"out": 1, "m_out": 1}, same=(("out", "x"), ("m_out", "m1"))),
    "unipc": _form("unipc_update", "x eu et last hist order out coef", 12, {"out": 1, "last": 1, "hist": None}),
    "ancestral": _form("ancestral_update", "x eu et z out coef", 3, {"out": 1}, optional=("et", "z")),
    "heun": _form("heun_update", "x eu et S D out coef", 5, {"out": 1, "S": 1, "D": 1}),
    "dpm2": _form("dpm2_update", "x eu et z S out coef", 5, {"out": 1, "S": 1}, optional=("et", "z")),
    "plms": _form("plms_update", "x eu et P H out coef", 12, {"out": 1, "P": 1, "H": 3}),
}
