"""Records tests/golden/sega/loops.npz: the end latents of the reference's OWN SemanticStableDiffusionPipeline (the unmodified
pipelines/semantic_stable_diffusion/pipeline_semantic_stable_diffusion.py, loaded through oracle/reference_runner.py with its own
schedulers) around the closed-form stand-in U-Net of tests/sega_cases.py, 5 steps, 2 x 4 x 8 x 8 latents. Data only.
tests/test_sega_host.py holds the restatement (tests/sega_ref.py) to it. Needs the reference checkout.

Supplied here at run time, nothing under oracle/ changes: ``paddle.nan_to_num`` and ``paddle.index_select`` as attributes of the shim
module; a bare ``ppdiffusers.pipelines.semantic_stable_diffusion`` package whose ``__path__`` is the reference's directory; stand-in
``tokenizer`` / ``text_encoder`` objects that map a prompt string to a row of tests/sega_cases.py's embedding table."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import reference_runner as rr   # noqa: E402
from tests import sega_cases as C   # noqa: E402
from tests.reference_cases import _FakeVAE   # noqa: E402

REF_SCHED = {"euler": ("scheduling_euler_discrete", "EulerDiscreteScheduler", {}),
             "ddim": ("scheduling_ddim", "DDIMScheduler", dict(clip_sample=False, set_alpha_to_one=False, steps_offset=1)),
             "dpm": ("scheduling_dpmsolver_multistep", "DPMSolverMultistepScheduler", {}),
             "heun": ("scheduling_heun_discrete", "HeunDiscreteScheduler", {})}


def reference_module():
    rr.ref_pipeline("pipeline_stable_diffusion")   # installs the shim and the stubbed plumbing
    import paddle
    from oracle import paddle_shim
    T = paddle_shim.Tensor
    paddle.nan_to_num = lambda x: T(torch.nan_to_num(x.t))
    paddle.index_select = lambda x, index, axis=0: T(torch.index_select(x.t, axis, index.t.long()))
    pkg = "ppdiffusers.pipelines.semantic_stable_diffusion"
    m = types.ModuleType(pkg)
    m.__path__ = [os.path.join(rr.REF_ROOT, "ppdiffusers", "pipelines", "semantic_stable_diffusion")]
    sys.modules[pkg] = m
    import importlib
    return importlib.import_module(pkg + ".pipeline_semantic_stable_diffusion")


class Tokenizer:
    """a prompt string -> its index in tests/sega_cases.py VOCAB, as a [len, 1] id tensor"""
    model_max_length = 77

    def __call__(self, prompts, **kw):
        prompts = [prompts] if isinstance(prompts, str) else list(prompts)
        return types.SimpleNamespace(input_ids=rr.to_shim(torch.tensor([[C.VOCAB[p]] for p in prompts])))


class TextEncoder:
    dtype = torch.float32

    def __init__(self):
        self.table = C.embedding_table()

    def __call__(self, input_ids, **kw):
        return (rr.to_shim(self.table[rr.from_shim(input_ids)[:, 0]]),)


class Bridge:
    def __init__(self, model):
        self._m, self.config, self.dtype = model, model.config, model.dtype

    def __call__(self, *a, **k):
        k = {n: rr.from_shim(v) for n, v in k.items()}
        return types.SimpleNamespace(sample=rr.to_shim(self._m(*rr.from_shim(a), **k)[0]))


def main():
    pm = reference_module()
    out = {}
    for name, (sched, n, use_sem, edit) in C.GOLDEN.items():
        mod, cls, kw = REF_SCHED[sched]
        scheduler = getattr(rr.ref_module(mod, "schedulers"), cls)(**C.SCHED, **kw)
        unet = Bridge(C.FormulaUNet(rr.FrozenConfig(in_channels=4, sample_size=C.HW)))
        pipe = pm.SemanticStableDiffusionPipeline(vae=_FakeVAE(rr, scaling_factor=0.18215, latent_channels=4), text_encoder=TextEncoder(),
                                                  tokenizer=Tokenizer(), unet=unet, scheduler=scheduler, safety_checker=None,
                                                  feature_extractor=None, requires_safety_checker=False)
        lat, sem = C.loop_inputs(n)[3:]
        res = pipe(prompt=list(C.PROMPTS), negative_prompt=list(C.NEGATIVE), editing_prompt=list(C.CONCEPTS[:n]), height=8 * C.HW,
                   width=8 * C.HW, num_inference_steps=C.GOLDEN_STEPS.get(name, C.STEPS), guidance_scale=C.GS, latents=rr.to_shim(lat.clone()), output_type="latent",
                   return_dict=False, sem_guidance=[rr.to_shim(s) for s in sem] if use_sem else None, **edit)[0]
        out[name] = rr.from_shim(res).numpy().astype(np.float32)
        print(name, out[name].shape, float(np.abs(out[name]).max()))
    os.makedirs(os.path.join(ROOT, "tests", "golden", "sega"), exist_ok=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "sega", "loops.npz"), **out)


if __name__ == "__main__":
    main()
