"""What the T2I-Adapter tests share: the U-Net configurations, the pairing of adapter and U-Net, seeded inputs, and the cases recorded
from the reference under tests/golden/adapter/ (scripts/make_adapter_golden.py)."""
import os

import numpy as np
import torch

from tests import adapter_ref as AR
from tests.configs import MINI_XL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "adapter")

# SD-1.5's structure in miniature (tests/configs.py SD15: three CrossAttnDownBlock2D and a DownBlock2D, the default block types), one
# layer per block: four sites, the last one a DownBlock2D without a downsampler
MINI_SD15 = dict(block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, attention_head_dim=8, layers_per_block=1,
                 norm_num_groups=32, sample_size=16)
# name -> (U-Net config, adapter name, latent pixels per adapter-feature pixel at the first site, L)
UNETS = {"sd15": (MINI_SD15, "full", 1, 7), "xl": (MINI_XL, "xl", 2, 77)}


def unet_inputs(cfg, B, H, W, L, seed=0):
    g = torch.Generator().manual_seed(seed)
    sample = torch.randn(B, 4, H, W, generator=g)
    enc = torch.randn(B, L, cfg["cross_attention_dim"], generator=g)
    added = None
    if cfg.get("addition_embed_type") == "text_time":
        td = cfg["projection_class_embeddings_input_dim"] - 6 * cfg["addition_time_embed_dim"]
        added = dict(text_embeds=torch.randn(B, td, generator=g), time_ids=torch.tensor([[1024., 1024., 0., 0., 1024., 1024.]]).repeat(B, 1))
    return sample, enc, added


def residuals(cfg, B, H, W, seed=7, scale=1.0, extra=0):
    """seeded O(1) residuals of the shapes an adapter's four features have for this U-Net -- the SD-1.5 shape: one per down block; the
    XL shape: one per down block and the mid block's --, `extra` more of the mid output's shape behind them"""
    g = torch.Generator().manual_seed(seed)
    shapes = AR.intrablock_shapes(cfg, B, H, W)
    return [scale * torch.randn(*s, generator=g) for s in shapes[:4] + [shapes[-1]] * extra]


def rounded(P, dtype=torch.bfloat16):
    """the parameters as the device holds them: matrices rounded to the element type, biases fp32"""
    return {k: (v.to(dtype).float() if v.dim() > 1 else v) for k, v in P.items()}


def image(B, C, H, W, seed=11):
    return torch.rand(B, C, H, W, generator=torch.Generator().manual_seed(seed))


# ---- the cases recorded from the reference (even geometries only: the shim's AvgPool2D has no ceil mode) ----
ADAPTER_GOLDEN = {"full": (2, 64, 64), "xl": (2, 64, 64), "light": (2, 64, 64)}       # name -> (B, H, W) of the image
UNET_GOLDEN = {"sd15": (2, 16, 16), "xl": (2, 16, 16)}                                  # name -> (B, H, W) of the latents
T = 501


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def unet_golden_inputs(name):
    from paddlemix_amd.unet import synth_unet_params
    cfg, _, _, L = UNETS[name]
    B, H, W = UNET_GOLDEN[name]
    P = synth_unet_params(cfg, seed=1234)
    return cfg, P, unet_inputs(cfg, B, H, W, L), residuals(cfg, B, H, W, scale=0.5, extra=1)


def unet_golden_forms(res, n_down):
    """name -> the residual list of each recorded form (the last entry of `res` is the extra one of the mid output's shape; the
    surplus one has no site's shape, so it is ignored wherever it ends up)"""
    four = res[:4]
    return dict(intrablock=four, too_few=four[:2], down_only=four[:n_down], surplus=four + [torch.ones(1, 1, 1, 1)],
                mid_extra=four + [res[4]])
