"""What the eight fused-step test families (guidance, multistep, unipc, ancestral, heun, dpm2, plms, singlestep) share on the host -- TEST
INFRASTRUCTURE ONLY: the start of every case's inputs, and the stand-ins a loop test puts around the model and the scheduler. Each
family's *_bounds.py keeps its own float64 reference, bound, schedule rows and cases."""
import functools

import torch


def base_inputs(name, spec):
    """The part of a case's inputs every family draws first and alike: (g, shape, x, eu, et), CPU fp32 [batch, n], from a generator
    seeded by the case's NAME (the family goes on drawing its state from g). kind="offset": a standard deviation 6400 times below
    the mean, what cancels in sum v^2 - n m^2. cfg=False: et is None (no guidance) -- drawn all the same, so x and eu do not move."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    shape = (spec["batch"], spec["n"])
    x = 3.0 * torch.randn(shape, generator=g)
    if spec.get("kind") == "offset":
        eu, et = 64.0 + 1e-2 * torch.randn(shape, generator=g), 64.0 + 1e-2 * torch.randn(shape, generator=g)
    else:
        eu = torch.randn(shape, generator=g)
        et = eu + 0.3 * torch.randn(shape, generator=g)
    return g, shape, x, eu, et if spec.get("cfg", True) else None


class Recording:
    """a UNet wrapper that keeps every model output of a run (what Replay then returns)"""

    def __init__(self, unet):
        self.unet, self.config, self._lib, self._emulated, self.outs = unet, unet.config, unet._lib, unet._emulated, []

    def __call__(self, *args, **kwargs):
        out = self.unet(*args, **kwargs)
        self.outs.append(out[0].detach().clone())
        return out


class Replay:
    """stands in the `unet` slot of the generic loop: returns the recorded outputs in order, as `dtype`, whatever the input"""

    def __init__(self, config, outs, dtype=torch.float64):
        self.config, self.outs, self.dtype, self.i = config, outs, dtype, 0

    def __call__(self, *args, **kwargs):
        self.i += 1
        return (self.outs[self.i - 1].to(self.dtype),)


def counting(sch, widen=False):
    """``sch`` with ``step`` counted in ``sch.step_calls``. widen (a scheduler whose step draws noise): for the generic loop run in
    FLOAT64. torch.randn draws other numbers in float64 than in float32 from the same seed, so a float64 model output would get noise
    the fused loop never saw; the wrapped step draws what ``step`` draws for the fused loop's dtype -- float32, the same call on the
    same generator -- and hands it over widened, through the ``noise=`` extension. Everything else of the generic loop is the
    pipeline's own."""
    sch.step_calls = 0
    step = sch.step

    @functools.wraps(step)   # (the pipeline reads step's signature to decide whether it takes a generator)
    def counted(model_output, timestep, sample, *args, **kwargs):
        sch.step_calls += 1
        if widen and kwargs.get("noise") is None:
            kwargs["noise"] = torch.randn(model_output.shape, generator=kwargs.get("generator"), device=model_output.device,
                                          dtype=torch.float32).double()
        return step(model_output, timestep, sample, *args, **kwargs)
    sch.step = counted
    return sch
