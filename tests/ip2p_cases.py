"""The cases of the InstructPix2Pix tests (tests/test_ip2p_host.py, tests/ip2p_child.py, tests/test_gpu_ip2p.py) -- TEST
INFRASTRUCTURE ONLY: the kernel matrices of the two entries, the miniature 8-channel U-Nets and the inputs of the loop tests."""
import torch

from paddlemix_amd import schedulers as S
from tests import configs
from tests.ip2p_bounds import RESIDENT

GS, GI, GR = 7.5, 1.5, 0.7
SCHED = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SCHEDULERS = {"euler": lambda: S.EulerDiscreteScheduler(**SCHED), "euler_a": lambda: S.EulerAncestralDiscreteScheduler(**SCHED),
              "ddim": lambda: S.DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, **SCHED),
              "dpm": lambda: S.DPMSolverMultistepScheduler(**SCHED), "heun": lambda: S.HeunDiscreteScheduler(**SCHED)}
SIGMA_SPACE = ("euler", "euler_a", "heun")   # have ``sigmas`` before set_timesteps, which is when the reference asks (SD :307)

# ---- mi355x_sd_guidance3, flat form: batch x per_sample of the issue; "off4": every pointer 4 bytes off a 16-byte boundary
FLAT = {f"b{b} n{n}{' off4' if off else ''}": dict(batch=b, n=n, off=off)
        for b in (1, 3) for n in (2, 5, 4 * 257 + 3, 4 * 4 * 9 * 11) for off in (0,)}
FLAT["b3 n1584 off4"] = dict(batch=3, n=4 * 4 * 9 * 11, off=1)
# ---- rescale forms: both sides of the size at which the kernel stops keeping a sample in registers, and 2; inputs with a common
# offset of 50 (eps form: the model outputs; x0 form: the latents), which a one-pass variance fails
RESCALE = {f"{form} n{n}{'' if s is None else f' sigma{s}'}": dict(batch=2, n=n, sigma=s)
           for form, sig in (("eps", (None,)), ("x0", (14.6, 0.03))) for s in sig for n in (2, 4 * 9 * 11, RESIDENT, RESIDENT + 1)}
# ---- mi355x_sd_ip2p_input
INPUT = {f"g{g} b{b} {cl}+{ci}x{h}x{w} {'one' if sc == 1.0 else 'sig'}": dict(groups=g, batch=b, c_lat=cl, c_img=ci, h=h, w=w, scale=sc)
         for g in (1, 3) for b in (1, 2) for cl, ci, h, w in ((4, 4, 8, 8), (4, 4, 9, 11), (4, 1, 3, 5))
         for sc in (1.0, 1.0 / (14.6 ** 2 + 1) ** 0.5)}

# ---- the loops: 8-channel miniatures of the SD-1.5 and the SDXL U-Net at latent 16 x 16 (GPU) / 8 x 8 (emulator), 4 steps
UNETS = {"tiny8": dict(configs.TINY, in_channels=8), "mini-xl8": dict(configs.MINI_XL, in_channels=8)}
STEPS = 4


def loop_inputs(cfg, batch=2, hw=8, tokens=7, seed=0):
    """(prompt_embeds, negative_prompt_embeds, image latents [batch, 4, hw, hw], initial noise, added, negative added), CPU fp32"""
    g = torch.Generator().manual_seed(seed)
    pe = torch.randn(batch, tokens, cfg["cross_attention_dim"], generator=g)
    ne = torch.randn(batch, tokens, cfg["cross_attention_dim"], generator=g)
    il = 3.0 * torch.randn(batch, 4, hw, hw, generator=g)   # (large enough for the image guidance scale to move the result)
    lat = torch.randn(batch, 4, hw, hw, generator=g)
    added = neg = None
    if cfg.get("addition_embed_type") == "text_time":
        td = cfg["projection_class_embeddings_input_dim"] - 6 * cfg["addition_time_embed_dim"]
        tids = torch.tensor([[128., 128., 0., 0., 128., 128.]]).repeat(batch, 1)
        added = dict(text_embeds=torch.randn(batch, td, generator=g), time_ids=tids)
        neg = dict(text_embeds=torch.randn(batch, td, generator=g), time_ids=tids)
    return pe, ne, il, lat, added, neg


# ---- the recorded runs of the reference's own pipelines (tests/golden/ip2p, scripts/make_ip2p_golden.py): a closed-form stand-in
# in the U-Net slot, so that the record holds the LOOP -- orders, the sigma-space question, the conversions, the rescale -- and nothing else
class FormulaUNet:
    """eps = 0.6 tanh(x_lat) + 0.25 x_img cos(t / 300) + 0.05 mean(text tokens) + 0.02 mean(text_embeds), fp32, on whatever the loop feeds it"""
    dtype = torch.float32

    def __init__(self, config):
        self.config = config

    def __call__(self, x, t, encoder_hidden_states=None, added_cond_kwargs=None, return_dict=False, **kw):
        c = torch.cos(torch.as_tensor(float(t), dtype=torch.float32) / 300.0)
        out = 0.6 * torch.tanh(x[:, :4]) + 0.25 * x[:, 4:] * c + 0.05 * encoder_hidden_states.mean(dim=(1, 2))[:, None, None, None]
        if added_cond_kwargs is not None:
            out = out + 0.02 * added_cond_kwargs["text_embeds"].mean(dim=1)[:, None, None, None]
        return (out,)


GOLDEN = {   # name: pipeline, scheduler, guidance_rescale (the SD pipeline has none)
    "sd_euler": ("sd", "euler", 0.0), "sd_euler_a": ("sd", "euler_a", 0.0), "sd_ddim": ("sd", "ddim", 0.0), "sd_dpm": ("sd", "dpm", 0.0),
    "sdxl_euler_rescale": ("sdxl", "euler", GR), "sdxl_dpm_rescale": ("sdxl", "dpm", GR), "sdxl_ddim_rescale": ("sdxl", "ddim", GR),
    "sdxl_heun_rescale": ("sdxl", "heun", GR),
}
GOLDEN_SEED = 21
