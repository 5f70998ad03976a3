"""The form table of the fused step-tail entries (paddlemix_amd/step_forms.py; tests/step_forms.py is its short-named view) against
the ABI: every row against its declaration in include/mi355x_sd.h and its generated signature in paddlemix_amd/_lib.py -- a row that
drifts would have the binding, the wrappers, the loop, the emulators and the GPU children describe an entry that does not exist -- and,
on a machine without a device, every refusal the table implies against the built library: csrc/capi.hip refuses before anything
touches the device, so the rule can be asked there with addresses inside one host buffer."""
from ctypes import c_float, c_int, c_int64, c_void_p

import pytest
import torch

from paddlemix_amd import _lib, ops, step_forms
from tests.header_decls import declared
from tests.step_forms import FORMS, TAIL

CTYPES = {"const float*": c_void_p, "float*": c_void_p, "void*": c_void_p, "int": c_int, "float": c_float, "int64_t": c_int64}


def test_every_form_agrees_with_its_signature():
    assert list(FORMS) == list(step_forms.FORMS) and len(FORMS) == 8
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


@pytest.mark.parametrize("name", list(step_forms.FORMS))
def test_every_form_is_its_declaration_in_the_header(name):
    form = step_forms.FORMS[name]
    ret, params = declared()["mi355x_sd_" + form.entry]
    assert ret == "int" and [n for _, n in params] == list(form.operands + step_forms.TAIL + ("stream",))
    for kind, n in params[:len(form.operands)]:
        assert kind == ("int" if n == "order" else "float*" if n in form.written else "const float*"), (form.entry, kind, n)
    assert [kind for kind, _ in params[len(form.operands):]] == ["float", "float", "int", "int64_t", "void*"]
    restype, argtypes = _lib.SIGNATURES["mi355x_sd_" + form.entry]
    assert restype is c_int and list(argtypes) == [CTYPES[kind] for kind, _ in params]
    assert (restype, argtypes) == step_forms.signature(form)


# ---------------------------------------------------------------------------------------------------------------- refusals on the host
N, PLANES, ORDER = 4096, 16, 3
INT64_MAX = 2 ** 63 - 1


def refused_calls(form, base):
    """{what: arguments} of every call the row says must be refused, each one deviation from a valid call that is itself never made:
    batch 1, per_sample 4096, gs 7.5, gr 0.7 (order 3), the operands one spare plane apart in a buffer of 16 x 4096 floats at `base`"""
    pointers = [k for k in form.operands if k != "order"]
    planes = {k: form.written.get(k, 1) or ORDER for k in pointers}
    addr, slot = {}, 0
    for k in pointers:
        addr[k], slot = base + 4 * N * slot, slot + planes[k] + 1
    assert slot - 1 <= PLANES
    ok = dict(addr, order=ORDER, guidance_scale=7.5, guidance_rescale=0.7, batch=1, per_sample=N)

    def but(**kw):
        return tuple(kw.get(k, ok[k]) for k in form.operands + step_forms.TAIL) + (None,)
    calls = {f"null {k}": but(**{k: None}) for k in pointers if k not in form.optional}
    for w in form.written:
        for r in pointers:
            if r == w or (r == "coef" and not form.coef_overlaps):
                continue
            lap = form.align // 4 if r == "coef" and form.align > 4 else 1   # (an aligned coef: by the least it can move)
            calls[f"{r} on the last element of {w}"] = but(**{r: addr[w] + 4 * (planes[w] * N - lap)})
    for w, r in form.same:
        calls[f"{w} one element into {r}"] = but(**{w: addr[r] + 4})
    most = max(planes.values())
    calls.update({"batch 0": but(batch=0), "per_sample 0": but(per_sample=0), "per_sample 1 under the rescale": but(per_sample=1),
                  "one element past int64": but(per_sample=INT64_MAX // 4 // most + 1),
                  "far past int64": but(batch=2 ** 31 - 1, per_sample=2 ** 62)})
    if "order" in form.operands:
        calls.update({"order 0": but(order=0), "order 4": but(order=4)})
    if form.align > 4:
        calls["coef off its alignment"] = but(coef=addr["coef"] + 4)
    return calls


@pytest.mark.skipif(torch.cuda.is_available(), reason="with a device the GPU children's refusals ask the same rule on device buffers")
@pytest.mark.parametrize("name", list(step_forms.FORMS))
def test_every_refusal_of_the_table_is_refused_before_the_device(name):
    form, lib = step_forms.FORMS[name], _lib.load()
    buf = torch.full((PLANES * N,), 7.25)
    assert buf.data_ptr() % 16 == 0
    calls = refused_calls(form, buf.data_ptr())
    fn = getattr(lib, "mi355x_sd_" + form.entry)
    for what, args in calls.items():
        assert fn(*args) == 1, (form.entry, what)                                  # MI355X_SD_ERR_INVALID
        assert lib.mi355x_sd_last_error().startswith(b"mi355x_sd_" + form.entry.encode() + b":"), (form.entry, what)
    assert bool((buf == 7.25).all())
