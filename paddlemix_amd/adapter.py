"""MI355X-native T2I-Adapter: ``T2IAdapter`` and ``MultiAdapter`` (PPD/models/adapter.py).

The adapter turns a control image (sketch, depth, pose ...) into one feature map per U-Net down block, once per image; the U-Net adds
them as ``down_intrablock_additional_residuals`` (paddlemix_amd/unet.py ``intrablock_residual``) on every step. Parameters are taken
under the reference's state-dict names and Paddle layouts (``adapter.conv_in.*``, ``adapter.body.N.in_conv.*``,
``adapter.body.N.resnets.M.block1 / block2.*``, the light variant's ``adapter.body.N.out_conv.*``) and repacked once with the U-Net's
helpers. The forward is a static program of C-ABI launches per (B, H, W), like every model here:

    mi355x_sd_pixel_unshuffle  NCHW fp32 image -> NHWC rows of in_channels * r * r 16-bit elements            (adapter.py:306, :356, :484)
    mi355x_sd_conv3x3          conv_in (full variants), block1 of every resnet, block2 of the light resnet    (:307, :449, :570-572)
    mi355x_sd_avgpool2         the downsampling blocks' AvgPool2D(2, 2, ceil_mode=True)                       (:411, :537)
    mi355x_sd_linear           every 1 x 1 convolution: in_conv, block2 of the full resnet, out_conv; the resnet's ``h + x`` is the
                               residual input of its last contraction's epilogue                               (:415, :451, :539-541)
    mi355x_sd_relu             between block1 and block2, in place                                             (:450, :571)
    mi355x_sd_unpatchify       each block's output -> the fp32 NCHW tensor the U-Net takes
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Dict, List, Mapping, Optional, Sequence

import torch

from . import _lib
from .checkpoint import PretrainedMixin
from .program import DeviceProgram, PlanBuilder, _Plan, _V
from .unet import _UNetWeights

Tensor = torch.Tensor

ADAPTER_DEFAULTS = dict(in_channels=3, channels=(320, 640, 1280, 1280), num_res_blocks=2, downscale_factor=8,
                        adapter_type="full_adapter")
ADAPTER_TYPES = ("full_adapter", "full_adapter_xl", "light_adapter")


def normalize_adapter_config(config: Mapping) -> dict:
    """ctor arguments of T2IAdapter (adapter.py:244-264) and what the kernels ask of them"""
    cfg = dict(ADAPTER_DEFAULTS)
    cfg.update({k: v for k, v in config.items() if not k.startswith("_")})
    unknown = sorted(set(cfg) - set(ADAPTER_DEFAULTS))
    if unknown:
        raise ValueError(f"T2IAdapter: unknown config keys {unknown}")
    if cfg["adapter_type"] not in ADAPTER_TYPES:
        raise ValueError(f"Unsupported adapter_type: '{cfg['adapter_type']}'. Choose either 'full_adapter' or 'full_adapter_xl' or "
                         "'light_adapter'.")
    cfg["channels"] = tuple(int(c) for c in cfg["channels"])
    r, cin, ch = int(cfg["downscale_factor"]), int(cfg["in_channels"]), cfg["channels"]
    if r < 1 or cin < 1 or int(cfg["num_res_blocks"]) < 1 or not ch:
        raise ValueError("T2IAdapter: downscale_factor, in_channels, num_res_blocks must be >= 1 and channels non-empty")
    light = cfg["adapter_type"] == "light_adapter"
    if (cin * r * r) % 8:
        raise ValueError(f"T2IAdapter(mi355x): in_channels * downscale_factor^2 = {cin * r * r} must be a multiple of 8 (the contraction "
                         "width of the first convolution)")
    q = 32 if light else 8   # the light blocks run at channels // 4
    if any(c % q for c in ch):
        raise ValueError(f"T2IAdapter(mi355x): channels {ch} must be multiples of {q} for adapter_type {cfg['adapter_type']!r} (the "
                         "convolution kernels take channel counts that are multiples of 8)")
    return cfg


def _blocks(cfg: dict) -> List[tuple]:
    """(cin, cout, down) per body block: FullAdapter (adapter.py:309-317), FullAdapterXL (:359-367), LightAdapter (:486-495)"""
    ch, t = cfg["channels"], cfg["adapter_type"]
    if t == "full_adapter":
        return [(ch[0], ch[0], False)] + [(ch[i - 1], ch[i], True) for i in range(1, len(ch))]
    if t == "full_adapter_xl":
        return [(ch[0], ch[1], False) if i == 1 else (ch[1], ch[2], True) if i == 2 else (ch[i], ch[i], False) for i in range(len(ch))]
    first = cfg["in_channels"] * cfg["downscale_factor"] ** 2
    return [(first, ch[0], False)] + [(ch[i], ch[i + 1], True) for i in range(len(ch) - 1)] + [(ch[-1], ch[-1], True)]


def adapter_param_shapes(config: Mapping) -> Dict[str, tuple]:
    """name -> shape (Paddle layouts: conv OIHW) of the reference's state dict, in construction order"""
    cfg = normalize_adapter_config(config)
    light = cfg["adapter_type"] == "light_adapter"
    S: Dict[str, tuple] = {}

    def conv(name, i, o, k):
        S[name + ".weight"], S[name + ".bias"] = (o, i, k, k), (o,)

    if not light:
        conv("adapter.conv_in", cfg["in_channels"] * cfg["downscale_factor"] ** 2, cfg["channels"][0], 3)
    for n, (cin, cout, _) in enumerate(_blocks(cfg)):
        b = f"adapter.body.{n}"
        width = cout // 4 if light else cout
        if light or cin != cout:
            conv(b + ".in_conv", cin, width, 1)
        for j in range(cfg["num_res_blocks"]):
            conv(f"{b}.resnets.{j}.block1", width, width, 3)
            conv(f"{b}.resnets.{j}.block2", width, width, 3 if light else 1)
        if light:
            conv(b + ".out_conv", width, cout, 1)
    return S


def synth_adapter_params(config: Mapping, seed: int = 1234, device="cpu") -> Dict[str, Tensor]:
    """random init with synth_unet_params' conventions: conv N(0, 1 / fan_in), biases N(0, 0.02^2), one generator, construction order"""
    g = torch.Generator(device=device).manual_seed(seed)
    P: Dict[str, Tensor] = {}
    for name, shape in adapter_param_shapes(config).items():
        r = torch.randn(shape, generator=g, device=device)
        P[name] = r * 0.02 if name.endswith(".bias") else r / math.sqrt(shape[1] * shape[2] * shape[3])
    return P


class _AdapterWeights(_UNetWeights):
    """the U-Net's repacking helpers over the adapter's layers: 3 x 3 convolutions through ``put_conv`` (the 64-channel K blocks
    where Cin allows: conv_in's 64 / 192 / 256 / 768 inputs do), 1 x 1 convolutions as the [O, I] matrices ``mi355x_sd_linear`` takes"""

    def load(self) -> None:
        for name in self.shapes:
            if name.endswith(".weight"):
                self.put_conv(name[:-len(".weight")], name[:-len(".weight")])


class T2IAdapter(DeviceProgram, PretrainedMixin):
    """``T2IAdapter(config, params)(image)`` -> the list of feature maps, fp32 NCHW, that ``UNet2DConditionModel.forward`` takes as
    ``down_intrablock_additional_residuals`` (adapter.py:216-284). The model needs the built HIP library and a GPU (no CPU fallback)."""
    _param_shapes = staticmethod(adapter_param_shapes)

    def __init__(self, config: Mapping, params: Mapping[str, Tensor], device="cuda", use_graph: bool = True, profile: bool = False):
        self._init_backend(device, use_graph, profile)
        self.cfg = normalize_adapter_config(config)
        self.config = SimpleNamespace(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in self.cfg.items()})
        self._body = _blocks(self.cfg)
        self._light = self.cfg["adapter_type"] == "light_adapter"
        _AdapterWeights(self, params).load()

    def _shapes(self) -> Dict[str, tuple]:
        return adapter_param_shapes(self.cfg)

    @property
    def downscale_factor(self) -> int:
        """the factor of the initial pixel-unshuffle: image sizes must be multiples of it (adapter.py:279-284)"""
        return int(self.cfg["downscale_factor"])

    @property
    def total_downscale_factor(self) -> int:
        """adapter.py:319, :371, :497"""
        return self.downscale_factor * 2 ** sum(1 for _, _, down in self._body if down)

    def _build_plan(self, B, H, W) -> _Plan:
        cfg, lib, stream, light = self.cfg, self._lib, self._stream_ptr, self._light
        pb = PlanBuilder(self, B)
        plan, r, cin = pb.plan, self.downscale_factor, cfg["in_channels"]
        h, w_ = H // r, W // r
        plan.image = pb.persist((B, cin, H, W), torch.float32)
        widest = max([cin * r * r] + [c for _, c, _ in self._body])
        bufs = [pb.sc(f"ad{i}", 2 * B * h * w_ * widest) for i in range(3)]   # three row buffers, taken in turn
        turn = [0]

        def rows(n, c) -> _V:
            turn[0] = (turn[0] + 1) % 3
            return _V(bufs[turn[0]], n, c)

        x = rows(B * h * w_, cin * r * r)
        pb.emit(lib.mi355x_sd_pixel_unshuffle, (plan.image.data_ptr(), B, cin, H, W, r, x.p, x.ld, stream), "misc")
        if not light:
            y = rows(x.rows, cfg["channels"][0])
            pb.conv3(x, h, w_, "adapter.conv_in", y)
            x = y
        plan.features = []
        for n, (bin_, bout, down) in enumerate(self._body):
            b = f"adapter.body.{n}"
            if down:
                ho, wo = (h + 1) // 2, (w_ + 1) // 2
                y = rows(B * ho * wo, x.C)
                pb.emit(lib.mi355x_sd_avgpool2, (x.p, x.ld, B, h, w_, x.C, y.p, y.ld, stream), "misc")
                x, h, w_ = y, ho, wo
            if b + ".in_conv.w" in self.w:
                y = rows(x.rows, self.w[b + ".in_conv.w"].shape[0])
                pb.linear(x, b + ".in_conv", y)
                x = y
            for j in range(cfg["num_res_blocks"]):
                t, y = rows(x.rows, x.C), rows(x.rows, x.C)
                pb.conv3(x, h, w_, f"{b}.resnets.{j}.block1", t)
                pb.emit(lib.mi355x_sd_relu, (t.p, t.ld, t.p, t.ld, t.rows, t.C, stream), "misc")
                if light:
                    pb.conv3(t, h, w_, f"{b}.resnets.{j}.block2", y, R=x)
                else:
                    pb.linear(t, f"{b}.resnets.{j}.block2", y, R=x)
                x = y
            if light:
                y = rows(x.rows, bout)
                pb.linear(x, b + ".out_conv", y)
                x = y
            out = pb.persist((B, x.C, h, w_), torch.float32)
            pb.emit(lib.mi355x_sd_unpatchify, (x.p, x.ld, B, x.C, h, w_, 1, out.data_ptr(), stream), "misc")
            plan.features.append(out)
        plan = pb.finish()
        plan.out = plan.features[-1]
        plan.B, plan.H, plan.W = B, H, W
        return plan

    def _get_plan(self, B, H, W) -> _Plan:
        return self.plan_for((B, H, W), lambda: self._build_plan(B, H, W))

    def forward(self, x: Tensor) -> List[Tensor]:
        if x.dim() != 4 or x.shape[1] != self.cfg["in_channels"]:
            raise ValueError(f"T2IAdapter: expected an image of shape [B, {self.cfg['in_channels']}, H, W], got {tuple(x.shape)}")
        B, _, H, W = x.shape
        r = self.downscale_factor
        if H % r or W % r:
            raise ValueError(f"T2IAdapter: image height and width ({H}, {W}) must be multiples of downscale_factor = {r}")
        self.require_gpu(x)
        plan = self._get_plan(B, H, W)
        self.run_staged(plan, lambda nb: plan.image.copy_(x.to(torch.float32), non_blocking=nb))
        return [t.clone() for t in plan.features]

    __call__ = forward


class MultiAdapter:
    """Several adapters whose features are summed with weights (adapter.py:27-100): ``forward(xs, adapter_weights)`` with ``xs`` one image
    per adapter -- a list, or one tensor with the images concatenated along the channels, split by the adapters' ``in_channels``. The
    weighted sum is a torch add on the fp32 outputs: it runs once per image."""

    def __init__(self, adapters: Sequence[T2IAdapter]):
        adapters = list(adapters)
        if len(adapters) == 0:
            raise ValueError("Expecting at least one adapter")
        if len(adapters) == 1:
            raise ValueError("For a single adapter, please use the `T2IAdapter` class instead of `MultiAdapter`")
        first = adapters[0]
        for idx in range(1, len(adapters)):
            a = adapters[idx]
            if a.total_downscale_factor != first.total_downscale_factor or a.downscale_factor != first.downscale_factor:
                raise ValueError(
                    f"Expecting all adapters to have the same downscaling behavior, but got:\n"
                    f"adapters[0].total_downscale_factor={first.total_downscale_factor}\n"
                    f"adapters[0].downscale_factor={first.downscale_factor}\n"
                    f"adapter[`{idx}`].total_downscale_factor={a.total_downscale_factor}\n"
                    f"adapter[`{idx}`].downscale_factor={a.downscale_factor}")
        self.adapters, self.num_adapter = adapters, len(adapters)
        self.total_downscale_factor, self.downscale_factor = first.total_downscale_factor, first.downscale_factor

    def forward(self, xs, adapter_weights: Optional[Sequence[float]] = None) -> List[Tensor]:
        if torch.is_tensor(xs):
            widths = [a.cfg["in_channels"] for a in self.adapters]
            if xs.dim() != 4 or xs.shape[1] != sum(widths):
                raise ValueError(f"MultiAdapter: expected [B, {sum(widths)}, H, W] (the adapters' images along the channels), got "
                                 f"{tuple(xs.shape)}")
            xs = list(torch.split(xs, widths, dim=1))
        if len(xs) != self.num_adapter:
            raise ValueError(f"MultiAdapter: {self.num_adapter} adapters, {len(xs)} images")
        if adapter_weights is None:
            adapter_weights = [1 / self.num_adapter] * self.num_adapter
        if len(adapter_weights) != self.num_adapter:
            raise ValueError(f"MultiAdapter: {self.num_adapter} adapters, {len(adapter_weights)} adapter_weights")
        state = None
        for x, w, adapter in zip(xs, adapter_weights, self.adapters):
            features = adapter(x.contiguous())
            if state is None:
                state = [float(w) * f for f in features]
            else:
                if len(features) != len(state):
                    raise ValueError("MultiAdapter: the adapters return different numbers of features")
                for i, f in enumerate(features):
                    state[i] += float(w) * f
        return state

    __call__ = forward
