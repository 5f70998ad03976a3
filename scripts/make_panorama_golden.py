"""Records tests/golden/panorama/loops.npz: the end latents of the reference's OWN StableDiffusionPanoramaPipeline (the unmodified
pipelines/stable_diffusion/pipeline_stable_diffusion_panorama.py, loaded through oracle/reference_runner.py with its own schedulers)
around the closed-form stand-in U-Net of tests/sega_cases.py, 4 steps, at the three geometries of tests/panorama_cases.py. Data
only. tests/test_panorama_host.py holds the restatement (tests/panorama_ref.py) to it. Needs the reference checkout.

Supplied here at run time, nothing under oracle/ changes: ``DDIMScheduler`` as an attribute of the stubbed ``ppdiffusers.schedulers``
module (the pipeline file imports it for a type annotation); a stand-in ``text_encoder`` that only has a dtype (the embeddings are
passed in)."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import reference_runner as rr   # noqa: E402
from tests import panorama_cases as C   # noqa: E402
from tests.reference_cases import _FakeVAE   # noqa: E402

REF_SCHED = {"euler": ("scheduling_euler_discrete", "EulerDiscreteScheduler", {}),
             "ddim": ("scheduling_ddim", "DDIMScheduler", dict(clip_sample=False, set_alpha_to_one=False, steps_offset=1)),
             "dpm": ("scheduling_dpmsolver_multistep", "DPMSolverMultistepScheduler", {}),
             "heun": ("scheduling_heun_discrete", "HeunDiscreteScheduler", {}),
             "pndm": ("scheduling_pndm", "PNDMScheduler", dict(skip_prk_steps=True, steps_offset=1))}


def reference_module():
    rr.install()
    sys.modules["ppdiffusers.schedulers"].DDIMScheduler = rr.ref_module("scheduling_ddim", "schedulers").DDIMScheduler
    return rr.ref_pipeline("pipeline_stable_diffusion_panorama")


class Bridge:
    def __init__(self, model):
        self._m, self.config, self.dtype = model, model.config, model.dtype

    def __call__(self, *a, **k):
        k = {n: rr.from_shim(v) for n, v in k.items() if n != "cross_attention_kwargs"}
        return types.SimpleNamespace(sample=rr.to_shim(self._m(*rr.from_shim(a), **k)[0]))


def main():
    pm = reference_module()
    out = {}
    for name, (sched, shape_name, gs) in C.GOLDEN.items():
        shape, circular, vbs = C.SHAPES[shape_name]
        mod, cls, kw = REF_SCHED[sched]
        scheduler = getattr(rr.ref_module(mod, "schedulers"), cls)(**C.SCHED, **kw)
        unet = Bridge(C.FormulaUNet(rr.FrozenConfig(in_channels=4, sample_size=64)))
        pipe = pm.StableDiffusionPanoramaPipeline(vae=_FakeVAE(rr, scaling_factor=0.18215, latent_channels=4),
                                                  text_encoder=types.SimpleNamespace(dtype=torch.float32), tokenizer=None, unet=unet,
                                                  scheduler=scheduler, safety_checker=None, feature_extractor=None,
                                                  requires_safety_checker=False)
        pe, ne, lat = C.loop_inputs(shape)
        res = pipe(prompt_embeds=rr.to_shim(pe), negative_prompt_embeds=rr.to_shim(ne), height=8 * shape[2], width=8 * shape[3],
                   num_inference_steps=C.STEPS, guidance_scale=gs, view_batch_size=vbs, circular_padding=circular,
                   latents=rr.to_shim(lat.clone()), output_type="latent", return_dict=False)[0]
        out[name] = rr.from_shim(res).numpy().astype(np.float32)
        print(name, out[name].shape, float(np.abs(out[name]).max()), int((out[name] == 0).sum()), "zeros")
    os.makedirs(os.path.join(ROOT, "tests", "golden", "panorama"), exist_ok=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "panorama", "loops.npz"), **out)


if __name__ == "__main__":
    main()
