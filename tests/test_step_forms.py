"""The form table of the fused step-tail entries (tests/step_forms.py) against the ABI: a row that drifts from its signature in
paddlemix_amd/_lib.py would have the emulators, the GPU children and the loop tests describe an entry that does not exist."""
from ctypes import c_float, c_int, c_int64, c_void_p

from paddlemix_amd import _lib, ops
from tests.step_forms import FORMS, TAIL


def test_every_form_agrees_with_its_signature():
    for form in FORMS.values():
        _check(form)


def _check(form):
    restype, argtypes = _lib.SIGNATURES["mi355x_sd_" + form.entry]
    kinds = [c_int if k == "order" else c_void_p for k in form.operands] + [c_float, c_float, c_int, c_int64, c_void_p]
    assert restype is c_int and list(argtypes) == kinds, (form, argtypes)
    assert len(argtypes) == len(form.operands) + len(TAIL) + 1        # the operands, gs / gr / batch / per_sample, the stream
    assert callable(getattr(ops, form.entry))                         # the wrapper
    pointers = [k for k in form.operands if k != "order"]
    assert pointers[-1] == "coef" and form.width > 0
    assert set(form.written) < set(pointers) and set(form.optional) < set(pointers) and not set(form.written) & set(form.optional)
    assert all(w in form.written and r in pointers and r not in form.written for w, r in form.same)
    assert (None in form.written.values()) == ("order" in form.operands)   # a span of `order` planes needs the operand
