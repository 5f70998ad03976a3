"""Records tests/golden/ip2p/loops.npz: the end latents of the reference's OWN InstructPix2Pix pipelines (the unmodified
pipeline_stable_diffusion_instruct_pix2pix.py and pipeline_stable_diffusion_xl_instruct_pix2pix.py, loaded through
oracle/reference_runner.py with its schedulers) around the closed-form stand-in U-Net of tests/ip2p_cases.py, 4 steps, latents passed
as `image`. Data only. tests/test_ip2p_host.py holds the restatement (tests/ip2p_ref.py) to it. Needs the reference checkout."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import reference_runner as rr   # noqa: E402
from tests import ip2p_cases as C   # noqa: E402
from tests.reference_cases import _FakeVAE   # noqa: E402

REF_SCHED = {"euler": ("scheduling_euler_discrete", "EulerDiscreteScheduler", {}),
             "euler_a": ("scheduling_euler_ancestral_discrete", "EulerAncestralDiscreteScheduler", {}),
             "ddim": ("scheduling_ddim", "DDIMScheduler", dict(clip_sample=False, set_alpha_to_one=False, steps_offset=1)),
             "dpm": ("scheduling_dpmsolver_multistep", "DPMSolverMultistepScheduler", {}),
             "heun": ("scheduling_heun_discrete", "HeunDiscreteScheduler", {})}


class Bridge:
    def __init__(self, model):
        self._m, self.config, self.dtype = model, model.config, model.dtype
        self.add_embedding = type("E", (), {"linear_1": type("L", (), {"in_features": model.config.get("projection_class_embeddings_input_dim")})()})()

    def __call__(self, *a, **k):
        k = {n: ({kk: rr.from_shim(vv) for kk, vv in v.items()} if isinstance(v, dict) else rr.from_shim(v)) for n, v in k.items()
             if n != "cross_attention_kwargs"}
        return rr.to_shim(tuple(self._m(*rr.from_shim(a), **k)))


def main():
    out = {}
    for name, (pipe_kind, sched, gr) in C.GOLDEN.items():
        cfg = C.UNETS["tiny8" if pipe_kind == "sd" else "mini-xl8"]
        pe, ne, il, lat, added, neg = C.loop_inputs(cfg, seed=C.GOLDEN_SEED)
        mod, cls, kw = REF_SCHED[sched]
        scheduler = getattr(rr.ref_module(mod, "schedulers"), cls)(**C.SCHED, **kw)
        unet = Bridge(C.FormulaUNet(rr.FrozenConfig(**cfg)))
        gg = torch.Generator().manual_seed(7)
        common = dict(prompt_embeds=rr.to_shim(pe), negative_prompt_embeds=rr.to_shim(ne), image=rr.to_shim(il), latents=rr.to_shim(lat.clone()),
                      num_inference_steps=C.STEPS, guidance_scale=C.GS, image_guidance_scale=C.GI, output_type="latent", return_dict=False,
                      generator=lambda shape: torch.randn(shape, generator=gg))
        if pipe_kind == "sd":
            pm = rr.ref_pipeline("pipeline_stable_diffusion_instruct_pix2pix")
            pipe = pm.StableDiffusionInstructPix2PixPipeline(vae=_FakeVAE(rr, scaling_factor=0.18215, latent_channels=4),
                                                             text_encoder=type("TextEncoder", (), {"dtype": torch.float32})(), tokenizer=None,
                                                             unet=unet, scheduler=scheduler, safety_checker=None, feature_extractor=None,
                                                             requires_safety_checker=False)
            res = pipe(**common)[0]
        else:
            pm = rr.ref_pipeline("pipeline_stable_diffusion_xl_instruct_pix2pix", "pipelines.stable_diffusion_xl")
            td = added["text_embeds"].shape[1]
            te2 = type("TextEncoder2", (), {"config": rr.FrozenConfig(projection_dim=td), "dtype": torch.float32})()
            vae = _FakeVAE(rr, scaling_factor=0.13025, latent_channels=4, force_upcast=False)
            vae.dtype = rr.to_shim(il).dtype   # (prepare_image_latents casts the latents to it, :550-551)
            pipe = pm.StableDiffusionXLInstructPix2PixPipeline(vae=vae,
                                                               text_encoder=None, text_encoder_2=te2, tokenizer=None, tokenizer_2=None, unet=unet,
                                                               scheduler=scheduler)
            res = pipe(**common, pooled_prompt_embeds=rr.to_shim(added["text_embeds"]),
                       negative_pooled_prompt_embeds=rr.to_shim(neg["text_embeds"]), guidance_rescale=gr, height=64, width=64,
                       original_size=(128, 128), target_size=(128, 128))[0]
        out[name] = rr.from_shim(res).numpy().astype(np.float32)
        print(name, out[name].shape, float(np.abs(out[name]).max()))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ip2p", "loops.npz"), **out)


if __name__ == "__main__":
    main()
