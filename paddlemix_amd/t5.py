"""MI355X-native T5 encoder (``T5EncoderModel``): the third text encoder of Stable Diffusion 3
(``_get_t5_prompt_embeds``, pipelines/stable_diffusion_3/pipeline_stable_diffusion_3.py:213-262).

Mirrors PPD/transformers/t5/modeling.py (T5Stack.forward :946-1113 for the encoder, gated-gelu feed-forward): token
embedding, per block RMS-norm -> fused QKV projection (no bias) -> attention WITHOUT 1/sqrt(d) scaling and with the
shared relative position bias as the attention kernel's additive mask -> output projection + residual -> RMS-norm ->
fused [wi_0 | wi_1] projection -> gelu_new(wi_0) * wi_1 -> wo + residual; final RMS-norm. The relative position bias
[1, heads, S, S] (``compute_bias`` :293-306) is built on the host once per sequence length -- it is a table lookup of
S x S bucket indices. Runs once per prompt; no CPU fallback.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Dict, Mapping, Optional

import torch

from . import _lib
from .checkpoint import PretrainedMixin, Table
from .program import DeviceProgram, PlanBuilder, _Plan, _V

Tensor = torch.Tensor

T5_DEFAULTS = dict(vocab_size=32128, d_model=512, d_kv=64, d_ff=1024, num_layers=8, num_heads=6,
                   relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6,
                   feed_forward_proj="gated-gelu")


def normalize_config(config: Mapping) -> dict:
    cfg = dict(T5_DEFAULTS)
    cfg.update({k: v for k, v in config.items() if not k.startswith("_")})
    if cfg["feed_forward_proj"] != "gated-gelu":
        raise NotImplementedError(f"feed_forward_proj={cfg['feed_forward_proj']!r} (gated-gelu is implemented)")
    if cfg["d_kv"] % 8 or cfg["d_kv"] > 160 or cfg["d_model"] % 8 or cfg["d_model"] > 4096 or cfg["d_ff"] % 8:
        raise ValueError("unsupported geometry: d_kv multiple of 8 and <= 160, d_model <= 4096")
    return cfg


def t5_param_shapes(config: Mapping) -> Dict[str, tuple]:
    """name -> shape (Paddle layouts) of the encoder's parameters; names as in the reference checkpoints."""
    cfg = normalize_config(config)
    D, inner, Fd = cfg["d_model"], cfg["num_heads"] * cfg["d_kv"], cfg["d_ff"]
    S: Dict[str, tuple] = {"shared.weight": Table((cfg["vocab_size"], D))}
    for i in range(cfg["num_layers"]):
        b = f"encoder.block.{i}"
        for n in ("q", "k", "v"):
            S[f"{b}.layer.0.SelfAttention.{n}.weight"] = (D, inner)
        S[f"{b}.layer.0.SelfAttention.o.weight"] = (inner, D)
        if i == 0:
            S[f"{b}.layer.0.SelfAttention.relative_attention_bias.weight"] = Table((cfg["relative_attention_num_buckets"],
                                                                                     cfg["num_heads"]))   # nn.Embedding
        S[f"{b}.layer.0.layer_norm.weight"] = (D,)
        S[f"{b}.layer.1.DenseReluDense.wi_0.weight"] = (D, Fd)
        S[f"{b}.layer.1.DenseReluDense.wi_1.weight"] = (D, Fd)
        S[f"{b}.layer.1.DenseReluDense.wo.weight"] = (Fd, D)
        S[f"{b}.layer.1.layer_norm.weight"] = (D,)
    S["encoder.final_layer_norm.weight"] = (D,)
    return S


def synth_t5_params(config: Mapping, seed: int = 1234, device="cpu") -> Dict[str, Tensor]:
    g = torch.Generator(device=device).manual_seed(seed)
    P: Dict[str, Tensor] = {}
    for name, shape in t5_param_shapes(config).items():
        r = torch.randn(shape, generator=g, device=device)
        if name == "shared.weight":
            t = r
        elif name.endswith("relative_attention_bias.weight"):
            t = r * 0.5
        elif len(shape) == 1:
            t = 1.0 + r * 0.05
        else:
            t = r / shape[0] ** 0.5
        P[name] = t
    return P


def relative_position_bucket(relative_position: Tensor, num_buckets: int = 32, max_distance: int = 128) -> Tensor:
    """bidirectional ``_relative_position_bucket`` (modeling.py:246-291)"""
    num_buckets //= 2
    buckets = (relative_position > 0).long() * num_buckets
    rp = relative_position.abs()
    max_exact = num_buckets // 2
    large = max_exact + (torch.log(rp.float() / max_exact) / math.log(max_distance / max_exact)
                         * (num_buckets - max_exact)).long()
    large = torch.minimum(large, torch.full_like(large, num_buckets - 1))
    return buckets + torch.where(rp < max_exact, rp, large)


class T5EncoderOutput(SimpleNamespace):
    def __getitem__(self, i):
        return (self.last_hidden_state,)[i]


class T5EncoderModel(DeviceProgram, PretrainedMixin):
    _param_shapes = staticmethod(t5_param_shapes)

    def __init__(self, config: Mapping, params: Mapping[str, Tensor], device="cuda", use_graph: bool = True,
                 profile: bool = False):
        self._init_backend(device, use_graph, profile)
        self.cfg = normalize_config(config)
        self.config = SimpleNamespace(**self.cfg)
        self._load_weights(params)

    def _load_weights(self, params: Mapping[str, Tensor]) -> None:
        cfg, dev, W = self.cfg, self.device, self.w
        shapes = t5_param_shapes(cfg)
        if "shared.weight" not in params and "encoder.embed_tokens.weight" in params:   # tied weights (:1120)
            params = dict(params, **{"shared.weight": params["encoder.embed_tokens.weight"]})
        missing = [k for k in shapes if k not in params]
        if missing:
            raise KeyError(f"missing parameters: {missing[:5]}{'...' if len(missing) > 5 else ''}")

        def get(name):
            t = params[name]
            if tuple(t.shape) != shapes[name]:
                raise ValueError(f"{name}: expected shape {shapes[name]} (Paddle layout), got {tuple(t.shape)}")
            return t.to(device=dev, dtype=torch.float32)

        bf = lambda t: t.to(_lib.elem_dtype()).contiguous()  # noqa: E731
        W["tok"] = bf(get("shared.weight"))
        for i in range(cfg["num_layers"]):
            b = f"encoder.block.{i}"
            a = b + ".layer.0.SelfAttention."
            W[f"l{i}.qkv.w"] = bf(torch.cat([get(a + n + ".weight").t() for n in ("q", "k", "v")], 0))
            W[f"l{i}.o.w"] = bf(get(a + "o.weight").t())
            f = b + ".layer.1.DenseReluDense."
            W[f"l{i}.wi.w"] = bf(torch.cat([get(f + "wi_0.weight").t(), get(f + "wi_1.weight").t()], 0))
            W[f"l{i}.wo.w"] = bf(get(f + "wo.weight").t())
            W[f"l{i}.ln0"] = get(b + ".layer.0.layer_norm.weight").contiguous()
            W[f"l{i}.ln1"] = get(b + ".layer.1.layer_norm.weight").contiguous()
        W["lnf"] = get("encoder.final_layer_norm.weight").contiguous()
        W["rel_bias"] = get("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight").contiguous()

    def _position_bias(self, S: int) -> Tensor:
        cfg = self.cfg
        ctx = torch.arange(S, device=self.device)[:, None]
        mem = torch.arange(S, device=self.device)[None, :]
        bucket = relative_position_bucket(mem - ctx, cfg["relative_attention_num_buckets"],
                                          cfg["relative_attention_max_distance"])
        return self.w["rel_bias"][bucket].permute(2, 0, 1).contiguous()   # [heads, S, S] fp32

    def _build_plan(self, B: int, S: int) -> _Plan:
        cfg, lib, W = self.cfg, self._lib, self.w
        D, H, dk, Fd, n = cfg["d_model"], cfg["num_heads"], cfg["d_kv"], cfg["d_ff"], cfg["num_layers"]
        inner, eps = H * dk, float(cfg["layer_norm_epsilon"])
        rows = B * S
        pb = PlanBuilder(self, B)
        plan, persist, emit, stream = pb.plan, pb.persist, pb.emit, pb.stream

        def linear(a: _V, wkey, out: _V, R: Optional[_V] = None):
            pb.linear(a, wkey, out, bias=False, R=R)

        def rms(x: _V, wkey, out: _V):
            emit(lib.mi355x_sd_rmsnorm, (x.p, rows, D, D, W[wkey].data_ptr(), eps, out.p, D, stream), "ln")

        plan.ids = persist((rows,), torch.int32)
        bias = persist((H, S, S), torch.float32)
        bias.copy_(self._position_bias(S))
        plan.consts = [bias]       # filled here, read by every run (paddlemix_amd/export.py ships its contents)
        xa, xb, h, qkv, ao, wi, ff = (_V.of(persist((rows, C), _lib.elem_dtype())) for C in (D, D, D, 3 * inner, inner, 2 * Fd, Fd))
        plan.last = persist((rows, D), _lib.elem_dtype())
        emit(lib.mi355x_sd_embed_tokens, (plan.ids.data_ptr(), rows, S, W["tok"].data_ptr(), None, D, xa.p, D, stream), "misc")
        for i in range(n):
            rms(xa, f"l{i}.ln0", h)
            linear(h, f"l{i}.qkv", qkv)
            # T5 attention: no 1/sqrt(d) scaling, the relative-position bias [heads, S, S] shared by the batch items
            pb.sdpa(qkv.cols(0, inner), qkv.cols(inner, inner), qkv.cols(2 * inner, inner), ao, H, S, S, bias.data_ptr(), (0, S * S, S),
                    scale=1.0)
            linear(ao, f"l{i}.o", xb, R=xa)
            rms(xb, f"l{i}.ln1", h)
            linear(h, f"l{i}.wi", wi)
            emit(lib.mi355x_sd_gated_activation, (wi.p, 2 * Fd, ff.p, Fd, rows, Fd, 3, stream), "misc")
            linear(ff, f"l{i}.wo", xa, R=xb)
        rms(xa, "lnf", _V.of(plan.last))
        pb.finish()
        plan.out = plan.last
        return plan

    def _get_plan(self, B, S) -> _Plan:
        return self.plan_for((B, S), lambda: self._build_plan(B, S))

    def forward(self, input_ids: Tensor, attention_mask=None, output_hidden_states=None, return_dict: Optional[bool] = True):
        if input_ids is None:
            raise ValueError("You have to specify input_ids")
        if attention_mask is not None or output_hidden_states:
            raise NotImplementedError("attention_mask / output_hidden_states are not implemented (SD3 passes neither)")
        cfg = self.cfg
        ids = input_ids.reshape(-1, input_ids.shape[-1])
        B, S = ids.shape
        self.require_gpu(ids)
        if int(ids.min()) < 0 or int(ids.max()) >= cfg["vocab_size"]:
            raise ValueError("input_ids out of range of the token embedding")
        plan = self._get_plan(B, S)
        self.run_staged(plan, lambda nb: plan.ids.copy_(ids.reshape(-1).to(torch.int32), non_blocking=nb))
        last = plan.last.reshape(B, S, cfg["d_model"]).float()
        if not return_dict:
            return (last,)
        return T5EncoderOutput(last_hidden_state=last)

    __call__ = forward
