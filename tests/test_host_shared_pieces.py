"""The two host pieces every model and the SD loop share (no GPU): the stream crossing of paddlemix_amd/program.py, and the step tail
of StableDiffusionDenoiser -- which device entry a step calls, with which scalars, on which row of the coefficient table. The tail's
calls are compared with tests/golden/step_tail_calls.json, recorded from the loop as it was when it still spelled the fused step out
inside its body: ``table + 8 * i`` over the scheduler's WHOLE schedule for the (a, b) form, ``table + 20 * (i - first)`` over the
steps actually run for the multistep form. The cases of the other tails were recorded from the loop as it was when every tail still
spelled its own call out (``table + 48 * (i - first)``, ``20 * i``, ...); a call of theirs also keeps, for every pointer that is
neither the latents, the model output, the result nor the table row, the index of its first appearance among such pointers of the run:
a buffer the tail owns for the whole loop records as a constant, one that is allocated again shows up."""
import contextlib
import functools
import json
import os

import pytest
import torch

from paddlemix_amd import program
from paddlemix_amd.pipeline import StableDiffusionDenoiser
from paddlemix_amd.schedulers import (DPMSolverMultistepScheduler, DPMSolverSinglestepScheduler, EulerAncestralDiscreteScheduler,
                                      EulerDiscreteScheduler, HeunDiscreteScheduler, KDPM2AncestralDiscreteScheduler,
                                      KDPM2DiscreteScheduler, PNDMScheduler, UniPCMultistepScheduler)
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
from tests.abi_emulator import on_emulator
from tests.abi_emulator_ancestral import AncestralEmulator
from tests.abi_emulator_dpm2 import Dpm2Emulator
from tests.abi_emulator_heun import HeunEmulator
from tests.abi_emulator_plms import PlmsEmulator
from tests.abi_emulator_singlestep import SinglestepEmulator
from tests.abi_emulator_unipc import UniPCEmulator
from tests.configs import TINY
from tests.step_forms import FORMS

SCHED = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_tail_calls.json")


# ---------------------------------------------------------------------------------------------------------------- the crossing
class _Stream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_stream(self, other):
        self.log.append(f"{self.name} waits for {other.name}")


@pytest.fixture
def streams(monkeypatch):
    log = []
    caller, model = _Stream("caller", log), _Stream("model", log)

    @contextlib.contextmanager
    def current(stream):
        log.append(f"enter {stream.name}")
        try:
            yield
        finally:
            log.append(f"exit {stream.name}")

    def current_stream(device):
        log.append(f"current stream of {device}")
        return caller

    monkeypatch.setattr(torch.cuda, "current_stream", current_stream)
    monkeypatch.setattr(torch.cuda, "stream", current)
    return model, log


def test_crossing_waits_enters_exits_waits(streams):
    model, log = streams
    with program.crossing(model, "cuda:3"):
        log.append("body")
    assert log == ["current stream of cuda:3", "model waits for caller", "enter model", "body", "exit model", "caller waits for model"]


def test_crossing_without_a_stream_does_nothing(streams):
    _, log = streams
    with program.crossing(None, "cpu"):
        log.append("body")
    assert log == ["body"]


def test_an_exception_in_the_body_propagates_and_skips_the_trailing_wait(streams):
    model, log = streams
    with pytest.raises(KeyError, match="from the body"):
        with program.crossing(model, "cuda:0"):
            raise KeyError("from the body")
    assert log == ["current stream of cuda:0", "model waits for caller", "enter model", "exit model"]


# ---------------------------------------------------------------------------------------------------------------- the step tail
class _Calls(UniPCEmulator, AncestralEmulator, HeunEmulator, Dpm2Emulator, PlmsEmulator, SinglestepEmulator):
    """keeps every step-tail call: its scalars as passed, its pointers as offsets (the table row from the table's base) and, for a
    pointer to state or noise, as the index of its first appearance among the run's (``state``, in the operands' order)"""

    def __init__(self):
        super().__init__()
        self.table, self.tail, self.seen = None, [], []

    def _keep(self, fn, x, eu, et, out, coef, state=(), **scalars):
        assert out != x
        self.seen += [p for p in dict.fromkeys(state) if p is not None and p not in self.seen]
        self.tail.append(dict(fn=fn, coef_offset=coef - self.table.data_ptr(), et_minus_eu=None if et is None else et - eu, **scalars,
                              **(dict(state=[None if p is None else self.seen.index(p) for p in state]) if state else {})))

    def mi355x_sd_axpby(self, x, y, out, coef, n, stream):
        self._keep("axpby", x, y, None, out, coef, n=n, stream=stream)
        return super().mi355x_sd_axpby(x, y, out, coef, n, stream)

    def mi355x_sd_cfg_axpby(self, x, eu, et, out, coef, gs, n, stream):
        self._keep("cfg_axpby", x, eu, et, out, coef, gs=gs, n=n, stream=stream)
        return super().mi355x_sd_cfg_axpby(x, eu, et, out, coef, gs, n, stream)


def _kept(form):
    """the entry of `form` on _Calls: keeps the call, then runs the emulator's"""
    name = "mi355x_sd_" + form.entry

    def entry(self, *args):
        a = dict(zip(form.operands + ("gs", "gr", "batch", "per_sample", "stream"), args, strict=True))
        x, eu, et, out, coef = (a.pop(k) for k in ("x", "eu", "et", "out", "coef"))
        self._keep(form.entry, x, eu, et, out, coef, state=[a.pop(k) for k in form.operands if k in a and k != "order"], **a)
        return getattr(super(_Calls, self), name)(*args)
    return name, entry


for _form in FORMS.values():
    setattr(_Calls, *_kept(_form))

# name: (scheduler, the call's arguments, the launches of 3 steps)
CASES = {
    "no_cfg": (EulerDiscreteScheduler, dict(guidance_scale=1.0), 3),
    "cfg": (EulerDiscreteScheduler, dict(guidance_scale=7.5), 3),
    "cfg_rescale": (EulerDiscreteScheduler, dict(guidance_scale=7.5, guidance_rescale=0.7), 3),
    "cfg_img2img": (EulerDiscreteScheduler, dict(guidance_scale=7.5, strength=0.7), 2),                       # first = 1: rows 1, 2
    "multistep_img2img": (DPMSolverMultistepScheduler, dict(guidance_scale=7.5, guidance_rescale=0.7, strength=0.7), 2),   # rows 0, 1
    "multistep_no_cfg": (DPMSolverMultistepScheduler, dict(guidance_scale=1.0, guidance_rescale=0.7), 3),   # no text half, rescale 0.0
    "unipc_img2img": (UniPCMultistepScheduler, dict(guidance_scale=7.5, guidance_rescale=0.7, strength=0.7), 2),          # rows 0, 1
    "ancestral": (EulerAncestralDiscreteScheduler, dict(guidance_scale=7.5, generator=True), 3),   # a new noise plane every step
    "heun": (HeunDiscreteScheduler, dict(guidance_scale=7.5), 5),                                    # 2 n - 1 evaluations
    "dpm2": (KDPM2DiscreteScheduler, dict(guidance_scale=7.5), 5),                                   # a null noise
    "dpm2_ancestral": (KDPM2AncestralDiscreteScheduler, dict(guidance_scale=7.5, generator=True), 5),   # one noise buffer
    "plms": (functools.partial(PNDMScheduler, skip_prk_steps=True), dict(guidance_scale=7.5), 4),    # n + 1 evaluations
    "singlestep_img2img": (functools.partial(DPMSolverSinglestepScheduler, solver_order=3), dict(guidance_scale=7.5, strength=0.7), 2),
}


def tail_calls(case, monkeypatch, table_of=lambda plan: plan.coef):
    scheduler, kw, _ = CASES[case]
    kw = dict(kw)
    emu = _Calls()
    pipe = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, synth_unet_params(TINY, seed=1234), backend=emu),
                                   scheduler(**SCHED))
    plan_of = pipe._fused_plan

    def fused_plan(*args):
        plan = plan_of(*args)
        emu.table = table_of(plan)
        return plan

    pipe._fused_plan = fused_plan
    # every noise plane of the run stays alive to its end, so that a new plane cannot get the address of one already counted
    planes, randn = [], torch.randn
    monkeypatch.setattr(torch, "randn", lambda *a, **k: planes.append(randn(*a, **k)) or planes[-1])
    g = torch.Generator().manual_seed(0)
    pe, ne, lat0 = torch.randn(1, 7, 64, generator=g), torch.randn(1, 7, 64, generator=g), torch.randn(1, 4, 8, 8, generator=g)
    start = dict(image=lat0, generator=g) if "strength" in kw else dict(latents=lat0, generator=g) if kw.pop("generator", 0) else \
        dict(latents=lat0)
    out = pipe(pe, ne if kw["guidance_scale"] > 1.0 else None, num_inference_steps=3, **start, **kw)
    assert torch.isfinite(out).all()
    return emu.tail


@pytest.mark.parametrize("case", list(CASES))
def test_step_tail_calls_are_the_recorded_ones(case, monkeypatch):
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    got = tail_calls(case, monkeypatch)
    assert len(got) == CASES[case][2]
    for call, rec in zip(got, want):
        if "state" not in rec:   # recorded before the recorder kept ``state``, when it asserted this instead: one buffer, in place
            assert set(call.pop("state", [0])) == {0}
    assert got == want
