"""The two host pieces every model and the SD loop share (no GPU): the stream crossing of paddlemix_amd/program.py, and the step tail
of StableDiffusionDenoiser -- which device entry a step calls, with which scalars, on which row of the coefficient table. The tail's
calls are compared with tests/golden/step_tail_calls.json, recorded from the loop as it was when it still spelled the fused step out
inside its body: ``table + 8 * i`` over the scheduler's WHOLE schedule for the (a, b) form, ``table + 20 * (i - first)`` over the
steps actually run for the multistep form."""
import contextlib
import json
import os

import pytest
import torch

from paddlemix_amd import program
from paddlemix_amd.pipeline import StableDiffusionDenoiser
from paddlemix_amd.schedulers import DPMSolverMultistepScheduler, EulerDiscreteScheduler
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
from tests.abi_emulator import on_emulator
from tests.abi_emulator_multistep import MultistepEmulator
from tests.configs import TINY

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
class _Calls(MultistepEmulator):
    """keeps every step-tail call: its scalars as passed, its pointers as offsets (the table row from the table's base)"""

    def __init__(self):
        super().__init__()
        self.table, self.tail, self.history = None, [], None

    def _keep(self, fn, x, eu, et, out, coef, **scalars):
        assert out != x
        self.tail.append(dict(fn=fn, coef_offset=coef - self.table.data_ptr(), et_minus_eu=None if et is None else et - eu, **scalars))

    def mi355x_sd_axpby(self, x, y, out, coef, n, stream):
        self._keep("axpby", x, y, None, out, coef, n=n, stream=stream)
        return super().mi355x_sd_axpby(x, y, out, coef, n, stream)

    def mi355x_sd_cfg_axpby(self, x, eu, et, out, coef, gs, n, stream):
        self._keep("cfg_axpby", x, eu, et, out, coef, gs=gs, n=n, stream=stream)
        return super().mi355x_sd_cfg_axpby(x, eu, et, out, coef, gs, n, stream)

    def mi355x_sd_cfg_rescale_axpby(self, x, eu, et, out, coef, gs, gr, batch, per_sample, stream):
        self._keep("cfg_rescale_axpby", x, eu, et, out, coef, gs=gs, gr=gr, batch=batch, per_sample=per_sample, stream=stream)
        return super().mi355x_sd_cfg_rescale_axpby(x, eu, et, out, coef, gs, gr, batch, per_sample, stream)

    def mi355x_sd_multistep_update(self, x, eu, et, m_prev, out, m_out, coef, gs, gr, batch, per_sample, stream):
        self.history = self.history or m_prev
        assert m_prev == m_out == self.history   # one history buffer, updated in place, for the whole loop
        self._keep("multistep_update", x, eu, et, out, coef, gs=gs, gr=gr, batch=batch, per_sample=per_sample, stream=stream)
        return super().mi355x_sd_multistep_update(x, eu, et, m_prev, out, m_out, coef, gs, gr, batch, per_sample, stream)


CASES = {
    "no_cfg": (EulerDiscreteScheduler, dict(guidance_scale=1.0)),
    "cfg": (EulerDiscreteScheduler, dict(guidance_scale=7.5)),
    "cfg_rescale": (EulerDiscreteScheduler, dict(guidance_scale=7.5, guidance_rescale=0.7)),
    "cfg_img2img": (EulerDiscreteScheduler, dict(guidance_scale=7.5, strength=0.7)),                       # first = 1: rows 1, 2
    "multistep_img2img": (DPMSolverMultistepScheduler, dict(guidance_scale=7.5, guidance_rescale=0.7, strength=0.7)),   # rows 0, 1
    "multistep_no_cfg": (DPMSolverMultistepScheduler, dict(guidance_scale=1.0, guidance_rescale=0.7)),   # no text half, rescale 0.0
}


def tail_calls(case, table_of=lambda plan: plan.coef):
    scheduler, kw = CASES[case]
    emu = _Calls()
    pipe = StableDiffusionDenoiser(on_emulator(UNet2DConditionModel, TINY, synth_unet_params(TINY, seed=1234), backend=emu),
                                   scheduler(**SCHED))
    plan_of = pipe._fused_plan

    def fused_plan(*args):
        plan = plan_of(*args)
        emu.table = table_of(plan)
        return plan

    pipe._fused_plan = fused_plan
    g = torch.Generator().manual_seed(0)
    pe, ne, lat0 = torch.randn(1, 7, 64, generator=g), torch.randn(1, 7, 64, generator=g), torch.randn(1, 4, 8, 8, generator=g)
    start = dict(image=lat0, generator=g) if "strength" in kw else dict(latents=lat0)
    out = pipe(pe, ne if kw["guidance_scale"] > 1.0 else None, num_inference_steps=3, **start, **kw)
    assert torch.isfinite(out).all()
    return emu.tail


@pytest.mark.parametrize("case", list(CASES))
def test_step_tail_calls_are_the_recorded_ones(case):
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    got = tail_calls(case)
    assert len(got) == (2 if "strength" in CASES[case][1] else 3)
    assert got == want
