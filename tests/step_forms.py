"""The eight fused step-tail entries of include/mi355x_sd.h as the tests see them -- TEST INFRASTRUCTURE ONLY: the rows of the product's
table (paddlemix_amd/step_forms.py, where the fields are explained) under the short operand names the emulators' arithmetic uses. Read by
the emulators' argument rule (tests/abi_emulator_guidance.py step_args), the GPU children's harness (tests/step_child.py) and the loop
tests' recorder (tests/test_host_shared_pieces.py). tests/test_step_forms.py holds every row to the header and to its signature in
paddlemix_amd/_lib.py.

Every entry is  mi355x_sd_<entry>(<operands>, gs, gr, batch, n, stream)  and ops.<entry> is its wrapper."""
from paddlemix_amd import step_forms

# header name -> the emulators' name; "<entry>.<operand>" where one header name has two (UniPC's hist keeps its own)
SHORT = {"eps_uncond": "eu", "eps_text": "et", "m_prev": "m1", "noise": "z", "sample": "S", "deriv": "D", "park": "P",
         "plms_update.hist": "H", "singlestep_update.hist": "H", "guidance_scale": "gs", "guidance_rescale": "gr", "per_sample": "n"}
TAIL = tuple(SHORT.get(k, k) for k in step_forms.TAIL)   # what follows the operands in every signature (then the stream)


def _short(form):
    def s(k):
        return SHORT.get(f"{form.entry}.{k}", SHORT.get(k, k))
    return form._replace(operands=tuple(map(s, form.operands)), written={s(k): v for k, v in form.written.items()},
                         optional=tuple(map(s, form.optional)), same=tuple((s(w), s(r)) for w, r in form.same),
                         state={s(k): v for k, v in form.state.items()})


FORMS = {name: _short(form) for name, form in step_forms.FORMS.items()}
