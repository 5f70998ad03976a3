"""Plain-torch restatement of the reference's T2I-Adapter (PPD/models/adapter.py) and of the U-Net forward that takes its features
(PPD/models/unet_2d_condition.py:1078-1152) -- TEST INFRASTRUCTURE ONLY, like oracle/.

Parameters are the reference's state dict in Paddle layouts (conv OIHW), fp32 or fp64, on any device. Pooling is
``avg_pool2d(2, 2, ceil_mode=True, count_include_pad=False)``: Paddle's AvgPool2D(ceil_mode=True) with its exclusive=True default, a
window over the bottom / right edge averages what is inside. Pinned against the reference's own modules on the geometries whose pooled
sizes are all even (tests/golden/adapter/, scripts/make_adapter_golden.py); odd geometries are pinned by this file alone.

``unet_forward_intrablock`` is oracle/unet_ref.unet_forward with each residual added to the output of the piece that produces its
site (``transformer_2d`` / ``resnet_block`` / ``downsample`` are wrapped for the duration of the call, not copied)."""
import contextlib
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

from oracle import unet_ref as U
from paddlemix_amd.adapter import _blocks, adapter_param_shapes, normalize_adapter_config, synth_adapter_params  # noqa: F401

Tensor = torch.Tensor

# tiny configurations of the three adapter types: channel counts the kernels take, every structural branch of the reference
# (in_conv present / absent, downsampling blocks, the XL order of blocks, the light variant's quarter width and out_conv)
ADAPTERS = {
    "full": dict(in_channels=3, channels=(64, 128, 256, 256), num_res_blocks=2, downscale_factor=8, adapter_type="full_adapter"),
    "xl": dict(in_channels=3, channels=(64, 128, 256, 256), num_res_blocks=2, downscale_factor=16, adapter_type="full_adapter_xl"),
    "light": dict(in_channels=1, channels=(64, 128, 256), num_res_blocks=2, downscale_factor=8, adapter_type="light_adapter"),
}


def _conv(P, name, x, padding):
    return F.conv2d(x, P[name + ".weight"].to(x.dtype), P[name + ".bias"].to(x.dtype), padding=padding)


def adapter_forward(P: Dict[str, Tensor], config: dict, x: Tensor) -> List[Tensor]:
    """T2IAdapter.forward (adapter.py:266-273) -> FullAdapter (:321-337) / FullAdapterXL (:373-387) / LightAdapter (:499-512)"""
    cfg = normalize_adapter_config(config)
    light = cfg["adapter_type"] == "light_adapter"
    x = F.pixel_unshuffle(x.to(next(iter(P.values())).dtype), cfg["downscale_factor"])
    if not light:
        x = _conv(P, "adapter.conv_in", x, 1)
    features = []
    for n, (_, _, down) in enumerate(_blocks(cfg)):
        b = f"adapter.body.{n}"
        if down:   # AdapterBlock / LightAdapterBlock.forward (:427-435, :548-555)
            x = F.avg_pool2d(x, 2, 2, ceil_mode=True, count_include_pad=False)
        if b + ".in_conv.weight" in P:
            x = _conv(P, b + ".in_conv", x, 0)
        for j in range(cfg["num_res_blocks"]):   # AdapterResnetBlock / LightAdapterResnetBlock.forward (:459-462, :580-583)
            h = F.relu(_conv(P, f"{b}.resnets.{j}.block1", x, 1))
            x = _conv(P, f"{b}.resnets.{j}.block2", h, 1 if light else 0) + x
        if light:
            x = _conv(P, b + ".out_conv", x, 0)
        features.append(x)
    return features


def multi_adapter_forward(Ps: Sequence[Dict[str, Tensor]], configs: Sequence[dict], xs: Sequence[Tensor],
                          adapter_weights: Optional[Sequence[float]] = None) -> List[Tensor]:
    """MultiAdapter.forward (adapter.py:75-100)"""
    n = len(Ps)
    w = [1 / n] * n if adapter_weights is None else list(adapter_weights)
    state = None
    for P, c, x, wi in zip(Ps, configs, xs, w):
        f = adapter_forward(P, c, x)
        state = [wi * t for t in f] if state is None else [s + wi * t for s, t in zip(state, f)]
    return state


def intrablock_sites(config: dict) -> List[str]:
    """the parameter-name prefix of the piece whose output takes each residual, in the reference's pop order"""
    cfg = U.normalize_config(config)
    n, names = len(cfg["down_block_types"]), []
    for i, bt in enumerate(cfg["down_block_types"]):
        last = cfg["layers_per_block"][i] - 1
        if bt == "CrossAttnDownBlock2D":      # unet_2d_blocks.py:1211-1213: the last resnet / attention pair, before the downsampler
            names.append(f"down_blocks.{i}.attentions.{last}")
        elif i != n - 1:                      # unet_2d_condition.py:1114-1118: the DownBlock2D's output, after its downsampler
            names.append(f"down_blocks.{i}.downsamplers.0")
        else:
            names.append(f"down_blocks.{i}.resnets.{last}")
    return names


def intrablock_shapes(config: dict, B: int, H: int, W: int) -> List[tuple]:
    """the shape of each site's tensor, the mid block's last: what an adapter's features must have"""
    cfg = U.normalize_config(config)
    n, out, h, w = len(cfg["down_block_types"]), [], H, W
    for i, bt in enumerate(cfg["down_block_types"]):
        c = cfg["block_out_channels"][i]
        if bt != "CrossAttnDownBlock2D" and i != n - 1:
            h, w = (h + 1) // 2, (w + 1) // 2
            out.append((B, c, h, w))
        else:
            out.append((B, c, h, w))
            if i != n - 1:
                h, w = (h + 1) // 2, (w + 1) // 2
    return out + [(B, cfg["block_out_channels"][-1], h, w)]


def unet_forward_intrablock(P, config, sample, timestep, encoder_hidden_states, down_intrablock_additional_residuals=None,
                            down_block_additional_residuals=None, **kw) -> Tensor:
    """unet_2d_condition.py:1078-1152 with T2I-Adapter residuals: ``down_block_additional_residuals`` alone is the deprecated form
    (:1084-1094). One residual per down block while the list lasts (:1101-1102, :1115-1118), then the next one after the mid block if
    it has the mid output's shape (:1147-1152); the rest is ignored."""
    rest = down_intrablock_additional_residuals
    if rest is None:
        rest = down_block_additional_residuals
    rest = list(rest)
    sites = intrablock_sites(config)
    order = iter(sites)
    pending = [next(order, None)]

    def wrap(fn):
        def piece(P_, name, x, *a, **k):
            y = fn(P_, name, x, *a, **k)
            if name == pending[0]:                    # a down block's site: it pops if anything is left
                pending[0] = next(order, None)
                if rest:
                    y = y + rest.pop(0).to(y.dtype)
            elif name == "mid_block.resnets.1" and rest and tuple(rest[0].shape) == tuple(y.shape):
                y = y + rest.pop(0).to(y.dtype)
            return y
        return piece

    with contextlib.ExitStack() as stack:
        for nm in ("transformer_2d", "resnet_block", "downsample"):
            orig = getattr(U, nm)
            setattr(U, nm, wrap(orig))
            stack.callback(setattr, U, nm, orig)
        return U.unet_forward(P, config, sample, timestep, encoder_hidden_states, **kw)
