"""MI355X-native UNet2DConditionModel: the drop-in for the reference's denoising-step callable.

Mirrors the call contract of ``UNet2DConditionModel.forward``
(ppdiffusers/ppdiffusers/models/unet_2d_condition.py:809-1207; seam B1 of SURVEY.md 8b: what
``StableDiffusionPipeline.__call__`` invokes at pipeline_stable_diffusion.py:866-879):

    unet(sample[B,C,h,w], timestep, encoder_hidden_states[B,L,D], added_cond_kwargs=..., return_dict=False) -> (noise_pred,)

and exposes ``.config`` / ``.dtype`` the way the pipelines read them.  Parameters are taken under the
reference's parameter names and *Paddle* layouts (Linear weight [in,out], conv OIHW) and repacked once for the
kernels.  The forward itself is a static program of C-ABI kernel launches (include/mi355x_sd.h) built per input
geometry and replayed as a hipGraph; sequencing follows the reference block structure
(unet_2d_blocks.py:750-799, 1142-1223, 1280-1307, 2317-2414, 2470-2524; resnet.py:728-808;
transformer_2d.py:272-509; attention.py:376-489).

Layout decisions: activations are bf16 token rows [B*H*W, C] (== NHWC) with explicit row strides;
every skip connection is produced directly inside the buffer its up-block consumer reads ("concat by
construction", no copy); GEGLU, bias, time-embedding add, residual add and 1/output_scale_factor are GEMM
epilogues; q/k/v projections are fused into one GEMM; all resnet time_emb_proj layers are one GEMM per step.
"""
from __future__ import annotations

import math
import os
from types import SimpleNamespace
from typing import Dict, List, Mapping, Optional, Tuple

import torch

from . import _lib
from ._lib import GEGLU, OUT_F32, SDPA_LOG2, SILU
from .checkpoint import PretrainedMixin, Table
from .program import DeviceProgram, PlanBuilder, _Plan, _V

Tensor = torch.Tensor

UNET_DEFAULTS = dict(
    sample_size=None, in_channels=4, out_channels=4, center_input_sample=False, flip_sin_to_cos=True, freq_shift=0,
    down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
    mid_block_type="UNetMidBlock2DCrossAttn",
    up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
    only_cross_attention=False, block_out_channels=(320, 640, 1280, 1280), layers_per_block=2, downsample_padding=1,
    mid_block_scale_factor=1, act_fn="silu", norm_num_groups=32, norm_eps=1e-5, cross_attention_dim=1280,
    transformer_layers_per_block=1, attention_head_dim=8, use_linear_projection=False, addition_embed_type=None,
    addition_time_embed_dim=None, upcast_attention=False, resnet_time_scale_shift="default",
    resnet_out_scale_factor=1.0, time_embedding_type="positional", projection_class_embeddings_input_dim=None,
    time_cond_proj_dim=None, class_embed_type=None, num_class_embeds=None, class_embeddings_concat=False,
    encoder_hid_dim=None, encoder_hid_dim_type=None,
    ip_adapter_num_tokens=4,   # extension: ImageProjection.num_image_text_embeds, which the reference reads off the IP-Adapter
                               # checkpoint instead of the config (loaders/unet.py _load_ip_adapter_weights)
)
_ONLY_DEFAULT = dict(attention_type="default", conv_in_kernel=3, conv_out_kernel=3, dropout=(0.0, 0), data_format="NCHW",
                     mid_block_only_cross_attention=(None, False), reverse_transformer_layers_per_block=None,
                     resnet_out_scale_factor=(1.0, 1), resnet_pre_temb_non_linearity=(None, False),
                     addition_embed_type_num_heads=64)
_UNSUPPORTED_IF_SET = ("time_embedding_dim", "time_embedding_act_fn", "timestep_post_act",
                       "cross_attention_norm", "dual_cross_attention", "resnet_skip_time_act")


def normalize_config(config: Mapping) -> dict:
    """ctor-argument handling of unet_2d_condition.py:172-290 for the branches this implementation covers."""
    cfg = dict(UNET_DEFAULTS)
    cfg.update({k: v for k, v in config.items() if not k.startswith("_")})
    for k in _UNSUPPORTED_IF_SET:
        if cfg.get(k) not in (None, False):
            raise NotImplementedError(f"UNet2DConditionModel(mi355x): config {k}={cfg[k]!r} is not implemented")
    # ctor arguments of the reference (unet_2d_condition.py:172-226) that change the arithmetic and are built only at their
    # default value: a checkpoint whose config sets them differently must not load silently
    for k, default in _ONLY_DEFAULT.items():
        if k in cfg and cfg[k] not in (default if isinstance(default, tuple) else (default,)):
            raise NotImplementedError(f"UNet2DConditionModel(mi355x): config {k}={cfg[k]!r} is not implemented "
                                      f"(only {default!r})")
    # encoder_hid_proj (unet_2d_condition.py:300-335): the IP-Adapter image projection is built, text_proj / image_proj are not
    if cfg["encoder_hid_dim_type"] not in (None, "ip_image_proj"):
        raise NotImplementedError(f"UNet2DConditionModel(mi355x): encoder_hid_dim_type={cfg['encoder_hid_dim_type']!r} "
                                  "is not implemented")
    if cfg["encoder_hid_dim_type"] is not None and cfg["encoder_hid_dim"] is None:
        raise ValueError(f"`encoder_hid_dim` has to be defined when `encoder_hid_dim_type` is set to "
                         f"{cfg['encoder_hid_dim_type']}.")
    if cfg["encoder_hid_dim_type"] is None and cfg["encoder_hid_dim"] is not None:
        raise NotImplementedError("UNet2DConditionModel(mi355x): encoder_hid_dim without a type (text_proj) is not implemented")
    if cfg["time_embedding_type"] != "positional" or cfg["resnet_time_scale_shift"] != "default":
        raise NotImplementedError("only positional time embedding / default resnet time shift are implemented")
    if cfg["act_fn"] not in ("silu", "swish"):
        raise NotImplementedError("only SiLU resnets are implemented")
    if cfg["downsample_padding"] != 1:
        raise NotImplementedError("downsample_padding must be 1")
    if cfg["addition_embed_type"] not in (None, "text_time"):
        raise NotImplementedError(f"addition_embed_type={cfg['addition_embed_type']!r}")
    # class embedding (unet_2d_condition.py:354-382; same messages)
    ct = cfg["class_embed_type"]
    if ct not in (None, "timestep", "identity", "projection", "simple_projection"):
        raise ValueError(f"class_embed_type {ct!r}")
    if ct in ("projection", "simple_projection") and cfg["projection_class_embeddings_input_dim"] is None:
        raise ValueError(f"`class_embed_type`: '{ct}' requires `projection_class_embeddings_input_dim` be set")
    if cfg["class_embeddings_concat"] and cfg["addition_embed_type"] is not None:
        raise NotImplementedError("class_embeddings_concat together with addition_embed_type")
    # "Check inputs" of the reference's constructor (unet_2d_condition.py:247-281; same messages, same order)
    dbt, ubt = cfg["down_block_types"], cfg["up_block_types"]
    if len(dbt) != len(ubt):
        raise ValueError(f"Must provide the same number of `down_block_types` as `up_block_types`. `down_block_types`: {dbt}. "
                         f"`up_block_types`: {ubt}.")
    for key, shown, seq in (("block_out_channels", "block_out_channels", (list, tuple)), ("only_cross_attention", "only_cross_attention", (list, tuple)),
                            ("attention_head_dim", "num_attention_heads", (list, tuple)),   # num_attention_heads = attention_head_dim (:245)
                            ("attention_head_dim", "attention_head_dim", (list, tuple)), ("cross_attention_dim", "cross_attention_dim", (list,)),
                            ("layers_per_block", "layers_per_block", (list, tuple))):
        v = cfg[key]
        if isinstance(v, seq) and len(v) != len(dbt):
            raise ValueError(f"Must provide the same number of `{shown}` as `down_block_types`. `{shown}`: {v}. `down_block_types`: {dbt}.")
    n = len(cfg["down_block_types"])
    tup = lambda x: tuple(x) if isinstance(x, (list, tuple)) else (x,) * n  # noqa: E731
    cfg["block_out_channels"] = tuple(cfg["block_out_channels"])
    for k in ("layers_per_block", "transformer_layers_per_block", "cross_attention_dim", "only_cross_attention"):
        cfg[k] = tup(cfg[k])
    cfg["num_attention_heads"] = tup(cfg["attention_head_dim"])  # the naming quirk at unet_2d_condition.py:245
    if any(cfg["only_cross_attention"]):
        raise NotImplementedError("only_cross_attention")
    for b in tuple(cfg["down_block_types"]) + tuple(cfg["up_block_types"]):
        if b not in ("CrossAttnDownBlock2D", "DownBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"):
            raise NotImplementedError(f"block type {b}")
    if cfg["mid_block_type"] != "UNetMidBlock2DCrossAttn":
        raise NotImplementedError(f"mid_block_type {cfg['mid_block_type']}")
    if cfg["out_channels"] > 4:
        raise NotImplementedError("out_channels > 4")
    return cfg


# ---------------------------------------------------------------------------------------------------------------
# structure walk shared by the parameter inventory and the program builder
# ---------------------------------------------------------------------------------------------------------------
def _structure(cfg: dict, encoder_only: bool = False) -> List[tuple]:
    """Layer descriptors in execution order.
    ('resnet', name, cin, cout, scale) | ('attn', name, C, heads, layers, cross) | ('skip',) |
    ('down', name, C) | ('up', name, C) | ('cat', skip_channels)"""
    boc = cfg["block_out_channels"]
    n = len(boc)
    L: List[tuple] = [("skip",)]
    out_c = boc[0]
    for i, bt in enumerate(cfg["down_block_types"]):
        in_c, out_c = out_c, boc[i]
        for j in range(cfg["layers_per_block"][i]):
            L.append(("resnet", f"down_blocks.{i}.resnets.{j}", in_c if j == 0 else out_c, out_c, 1.0))
            if bt == "CrossAttnDownBlock2D":
                L.append(("attn", f"down_blocks.{i}.attentions.{j}", out_c, cfg["num_attention_heads"][i],
                          cfg["transformer_layers_per_block"][i], cfg["cross_attention_dim"][i]))
            L.append(("skip",))
        if i != n - 1:
            L.append(("down", f"down_blocks.{i}.downsamplers.0.conv", out_c))
            L.append(("skip",))
    ms = float(cfg["mid_block_scale_factor"])
    L.append(("resnet", "mid_block.resnets.0", boc[-1], boc[-1], ms))
    L.append(("attn", "mid_block.attentions.0", boc[-1], cfg["num_attention_heads"][-1],
              cfg["transformer_layers_per_block"][-1], cfg["cross_attention_dim"][-1]))
    L.append(("resnet", "mid_block.resnets.1", boc[-1], boc[-1], ms))
    if encoder_only:   # ControlNetModel: conv_in skip, down blocks, mid block
        return L
    rboc = tuple(reversed(boc))
    rlayers = tuple(reversed(cfg["layers_per_block"]))
    rtl = tuple(reversed(cfg["transformer_layers_per_block"]))
    rcross = tuple(reversed(cfg["cross_attention_dim"]))
    rheads = tuple(reversed(cfg["num_attention_heads"]))
    out_c = rboc[0]
    for i, bt in enumerate(cfg["up_block_types"]):
        prev_out, out_c = out_c, rboc[i]
        in_c = rboc[min(i + 1, n - 1)]
        nl = rlayers[i] + 1
        for j in range(nl):
            skip_c = in_c if j == nl - 1 else out_c
            rin = prev_out if j == 0 else out_c
            L.append(("cat", skip_c))
            L.append(("resnet", f"up_blocks.{i}.resnets.{j}", rin + skip_c, out_c, 1.0))
            if bt == "CrossAttnUpBlock2D":
                L.append(("attn", f"up_blocks.{i}.attentions.{j}", out_c, rheads[i], rtl[i], rcross[i]))
        if i != n - 1:
            L.append(("up", f"up_blocks.{i}.upsamplers.0.conv", out_c))
    return L


def intrablock_sites(layers: List[tuple]) -> List[int]:
    """Indices into a layer list of the layers whose output takes a T2I-Adapter residual, in the order the reference pops them
    (unet_2d_condition.py:1096-1119, 1146-1152): per down block the last attention of a CrossAttnDownBlock2D (unet_2d_blocks.py:1211-1213:
    before its downsampler) or the last layer of a DownBlock2D (after its downsampler, if it has one); then the mid block's last resnet"""
    last: Dict[int, int] = {}
    for i, d in enumerate(layers):
        if d[0] in ("resnet", "attn", "down") and d[1].startswith("down_blocks."):
            b = int(d[1].split(".")[1])
            has_attn = any(e[0] == "attn" and e[1].startswith(f"down_blocks.{b}.") for e in layers)
            if d[0] == "attn" or not has_attn:
                last[b] = i
    sites = [last[b] for b in sorted(last)]
    return sites + [i for i, d in enumerate(layers) if d[0] == "resnet" and d[1] == "mid_block.resnets.1"]


def unet_param_shapes(config: Mapping) -> Dict[str, tuple]:
    """name -> shape (Paddle layouts) of every parameter the configured UNet owns, in construction order
    (unet_2d_condition.py:287-631 and the block ctors in unet_2d_blocks.py)."""
    cfg = normalize_config(config)
    boc = cfg["block_out_channels"]
    ted = boc[0] * 4
    S: Dict[str, tuple] = {}

    def lin(name, i, o, bias=True):
        S[name + ".weight"] = (i, o)
        if bias:
            S[name + ".bias"] = (o,)

    def conv(name, i, o, k):
        S[name + ".weight"] = (o, i, k, k)
        S[name + ".bias"] = (o,)

    def norm(name, c):
        S[name + ".weight"] = (c,)
        S[name + ".bias"] = (c,)

    conv("conv_in", cfg["in_channels"], boc[0], 3)
    lin("time_embedding.linear_1", boc[0], ted)
    if cfg["time_cond_proj_dim"] is not None:   # TimestepEmbedding.cond_proj, no bias (embeddings.py:265-266)
        lin("time_embedding.cond_proj", cfg["time_cond_proj_dim"], boc[0], bias=False)
    lin("time_embedding.linear_2", ted, ted)
    ct, pdim = cfg["class_embed_type"], cfg["projection_class_embeddings_input_dim"]
    if ct is None and cfg["num_class_embeds"] is not None:
        S["class_embedding.weight"] = Table((cfg["num_class_embeds"], ted))   # nn.Embedding: never transposed
    elif ct in ("timestep", "projection"):                                     # TimestepEmbedding
        lin("class_embedding.linear_1", boc[0] if ct == "timestep" else pdim, ted)
        lin("class_embedding.linear_2", ted, ted)
    elif ct == "simple_projection":
        lin("class_embedding", pdim, ted)
    if cfg["addition_embed_type"] == "text_time":
        lin("add_embedding.linear_1", cfg["projection_class_embeddings_input_dim"], ted)
        lin("add_embedding.linear_2", ted, ted)
    ted_b = ted * (2 if cfg["class_embeddings_concat"] else 1)   # blocks_time_embed_dim (unet_2d_condition.py:443-449)
    for d in _structure(cfg):
        if d[0] == "resnet":
            _, name, cin, cout, _ = d
            norm(name + ".norm1", cin)
            conv(name + ".conv1", cin, cout, 3)
            lin(name + ".time_emb_proj", ted_b, cout)
            norm(name + ".norm2", cout)
            conv(name + ".conv2", cout, cout, 3)
            if cin != cout:
                conv(name + ".conv_shortcut", cin, cout, 1)
        elif d[0] == "attn":
            _, name, c, heads, layers, cross = d
            norm(name + ".norm", c)
            if cfg["use_linear_projection"]:
                lin(name + ".proj_in", c, c)
            else:
                conv(name + ".proj_in", c, c, 1)
            for l in range(layers):
                b = f"{name}.transformer_blocks.{l}"
                norm(b + ".norm1", c)
                for a, kd in ((".attn1", c), (".attn2", cross)):
                    lin(b + a + ".to_q", c, c, bias=False)
                    lin(b + a + ".to_k", kd, c, bias=False)
                    lin(b + a + ".to_v", kd, c, bias=False)
                    lin(b + a + ".to_out.0", c, c)
                    if a == ".attn1":
                        norm(b + ".norm2", c)
                    elif cfg["encoder_hid_dim_type"] == "ip_image_proj":   # IPAdapterAttnProcessor (attention_processor.py:1816-1817)
                        lin(b + a + ".processor.to_k_ip", kd, c, bias=False)
                        lin(b + a + ".processor.to_v_ip", kd, c, bias=False)
                norm(b + ".norm3", c)
                lin(b + ".ff.net.0.proj", c, 8 * c)
                lin(b + ".ff.net.2", 4 * c, c)
            if cfg["use_linear_projection"]:
                lin(name + ".proj_out", c, c)
            else:
                conv(name + ".proj_out", c, c, 1)
        elif d[0] in ("down", "up"):
            conv(d[1], d[2], d[2], 3)
    norm("conv_norm_out", boc[0])
    conv("conv_out", boc[0], cfg["out_channels"], 3)
    if cfg["encoder_hid_dim_type"] == "ip_image_proj":   # ImageProjection (embeddings.py:507-518); last, so other draws keep their order
        dx = cfg["cross_attention_dim"][0]
        lin("encoder_hid_proj.image_embeds", cfg["encoder_hid_dim"], cfg["ip_adapter_num_tokens"] * dx)
        norm("encoder_hid_proj.norm", dx)
    return S


def synth_unet_params(config: Mapping, seed: int = 1234, device="cpu", dtype=torch.float32, generator=None,
                      only: Optional[range] = None) -> Dict[str, Tensor]:
    """Random-init parameters (no checkpoints are available offline): conv/linear N(0, 1/fan_in), biases
    N(0, 0.02^2), norm gamma 1 + N(0, 0.02^2), beta N(0, 0.02^2); one generator, construction order.
    `generator` + `only`: draw just the parameters `only` indexes (a run of the construction order) from a generator the caller
    positioned there -- how a 2.6 B-parameter set is drawn as parallel shards (tests/parity_cases.py)."""
    g = generator if generator is not None else torch.Generator(device=device).manual_seed(seed)
    P: Dict[str, Tensor] = {}
    items = list(unet_param_shapes(config).items())
    for name, shape in (items if only is None else items[only.start:only.stop]):
        r = torch.randn(shape, generator=g, device=device)
        if name.endswith(".bias"):
            t = r * 0.02
        elif len(shape) == 1:
            t = 1.0 + r * 0.02
        elif len(shape) == 2:
            t = r / math.sqrt(shape[0])
        else:
            t = r / math.sqrt(shape[1] * shape[2] * shape[3])
        P[name] = t.to(dtype)
    return P


# ---------------------------------------------------------------------------------------------------------------
# weights and program: each a small object whose methods are the stages, under the names csrc/unet_weights.hip (Packer) and
# csrc/unet_plan.hip (Planner) use for the same stages -- a change to one has its counterpart in the stage of that name there
# ---------------------------------------------------------------------------------------------------------------
class _UNetWeights:
    """The reference's parameters (its names, Paddle layouts) repacked once for the kernels into ``model.w``. Stages: ``stem`` (conv_in
    and the embeddings), ``resnet``, ``transformer`` / ``transformer_block``, ``sampler``, ``batched`` (what the layers contribute to the
    one-GEMM-per-step matrices), ``head``."""

    def __init__(self, model: "UNet2DConditionModel", params: Mapping[str, Tensor]):
        self.m, self.cfg, self.W, self.params, self.shapes = model, model.cfg, model.w, params, model._shapes()
        missing = [k for k in self.shapes if k not in params]
        if missing:
            raise KeyError(f"missing parameters: {missing[:5]}{'...' if len(missing) > 5 else ''}")
        model._kb64 = set()
        model._log2_blocks = set()   # transformer blocks whose self-attention scores are base-2 exponents (fold_softmax_scale)
        model._temb_off, model._kv_off = {}, {}   # where a resnet's time_emb_proj / a block's to_k, to_v sit in temb_all / kv_all
        self.temb_w, self.temb_b = [], []
        self.kv_w, self.kvip_w = [], []            # every cross-attention to_k / to_v (IPAdapterAttnProcessor: to_k_ip / to_v_ip, same offsets)

    def load(self) -> None:
        self.stem()
        for d in self.m._layers:
            if d[0] == "resnet":
                self.resnet(d[1], d[2], d[3])
            elif d[0] == "attn":
                self.transformer(*d[1:5])
            elif d[0] in ("down", "up"):
                self.sampler(d[1])
        self.batched()
        self.head()

    def get(self, name):
        t = self.params[name]
        if tuple(t.shape) != self.shapes[name]:
            raise ValueError(f"{name}: shape {tuple(t.shape)} != expected {self.shapes[name]} (Paddle layout)")
        return t.to(device=self.m.device, dtype=torch.float32)

    @staticmethod
    def bf(t):
        return t.to(_lib.elem_dtype()).contiguous()

    def lin_w(self, name):  # Paddle [in,out] -> [out,in]
        return self.get(name + ".weight").t()

    def put_lin(self, key, name, bias=True):
        self.W[key + ".w"] = self.bf(self.lin_w(name))
        if bias:
            self.W[key + ".b"] = self.get(name + ".bias").contiguous()

    def put_conv(self, key, name):  # OIHW -> [O][kh][kw][I]; 3x3 with Cin % 64 == 0 -> [O][I/64][kh][kw][64] (MI355X_SD_CONV_KB64)
        w = self.get(name + ".weight")
        O, I, kh, kw = w.shape
        if kh == 3 and I % 64 == 0:
            self.W[key + ".w"] = self.bf(w.reshape(O, I // 64, 64, kh, kw).permute(0, 1, 3, 4, 2).reshape(O, -1))
            self.m._kb64.add(key)
        else:
            self.W[key + ".w"] = self.bf(w.permute(0, 2, 3, 1).reshape(O, -1))
        self.W[key + ".b"] = self.get(name + ".bias").contiguous()

    def put_conv_in(self, key, w, name):  # -> [ky][kx][ci][O], the conv_in kernel's layout
        self.W[key + ".w"] = self.bf(w.permute(2, 3, 1, 0).reshape(-1, w.shape[0]))
        self.W[key + ".b"] = self.get(name + ".bias").contiguous()

    def put_norm(self, key, name):
        self.W[key + ".g"] = self.get(name + ".weight").contiguous()
        self.W[key + ".b"] = self.get(name + ".bias").contiguous()

    def put_ln_lin(self, key, w, bias, norm):
        """LayerNorm `norm` folded into the projection w [N, K] (mi355x_sd_linear_ln): W' = W diag(gamma) in bf16,
        ws = row sums of the bf16 W' (what the MFMAs actually sum), b' = bias + W beta."""
        wp_ = self.bf(w * self.get(norm + ".weight")[None, :])
        self.W[key + ".w"] = wp_
        self.W[key + ".ws"] = wp_.float().sum(1).contiguous()
        bb = w @ self.get(norm + ".bias")
        self.W[key + ".b"] = (bb if bias is None else bias + bb).contiguous()

    # ---- stages ----
    def stem(self):
        cfg, put_lin = self.cfg, self.put_lin
        self.put_conv_in("conv_in", self.get("conv_in.weight"), "conv_in")
        put_lin("time_embedding.linear_1", "time_embedding.linear_1")
        put_lin("time_embedding.linear_2", "time_embedding.linear_2")
        if cfg["addition_embed_type"] == "text_time":
            put_lin("add_embedding.linear_1", "add_embedding.linear_1")
            put_lin("add_embedding.linear_2", "add_embedding.linear_2")
        if cfg["time_cond_proj_dim"] is not None:
            put_lin("time_embedding.cond_proj", "time_embedding.cond_proj", bias=False)
        if self.m._class_kind == "embedding":
            self.W["class_embedding.table"] = self.bf(self.get("class_embedding.weight"))
        elif self.m._class_kind in ("timestep", "projection"):
            put_lin("class_embedding.linear_1", "class_embedding.linear_1")
            put_lin("class_embedding.linear_2", "class_embedding.linear_2")
        elif self.m._class_kind == "simple_projection":
            put_lin("class_embedding", "class_embedding")
        if self.m._ip:
            put_lin("encoder_hid_proj.image_embeds", "encoder_hid_proj.image_embeds")
            self.put_norm("encoder_hid_proj.norm", "encoder_hid_proj.norm")

    def resnet(self, name, cin, cout):
        self.put_norm(name + ".norm1", name + ".norm1")
        self.put_conv(name + ".conv1", name + ".conv1")
        self.m._temb_off[name] = sum(w.shape[0] for w in self.temb_w)
        self.temb_w.append(self.lin_w(name + ".time_emb_proj"))
        self.temb_b.append(self.get(name + ".time_emb_proj.bias"))
        self.put_norm(name + ".norm2", name + ".norm2")
        self.put_conv(name + ".conv2", name + ".conv2")
        if cin != cout:
            self.put_conv(name + ".conv_shortcut", name + ".conv_shortcut")

    def transformer(self, name, c, heads, layers):
        self.put_norm(name + ".norm", name + ".norm")
        put = self.put_lin if self.cfg["use_linear_projection"] else self.put_conv
        put(name + ".proj_in", name + ".proj_in")
        put(name + ".proj_out", name + ".proj_out")
        for l in range(layers):
            self.transformer_block(f"{name}.transformer_blocks.{l}", c, heads)

    def transformer_block(self, b, c, heads):
        m, W, lin_w, get = self.m, self.W, self.lin_w, self.get
        wq = lin_w(b + ".attn1.to_q")
        if m.fold_scale and c // heads == 64:
            wq = wq * ((c // heads) ** -0.5 * 1.4426950408889634)
            m._log2_blocks.add(b)
        wqkv = torch.cat([wq, lin_w(b + ".attn1.to_k"), lin_w(b + ".attn1.to_v")], 0)
        if m.fold_ln:
            self.put_ln_lin(b + ".attn1.qkv", wqkv, None, b + ".norm1")
            self.put_ln_lin(b + ".attn2.q", lin_w(b + ".attn2.to_q"), None, b + ".norm2")
        else:
            for nm in (".norm1", ".norm2", ".norm3"):
                self.put_norm(b + nm, b + nm)
            W[b + ".attn1.qkv.w"] = self.bf(wqkv)
            W[b + ".attn2.q.w"] = self.bf(lin_w(b + ".attn2.to_q"))
        self.put_lin(b + ".attn1.out", b + ".attn1.to_out.0")
        if any(x != self.cfg["cross_attention_dim"][0] for x in self.cfg["cross_attention_dim"]):
            raise NotImplementedError("per-block cross_attention_dim")
        m._kv_off[b] = sum(w.shape[0] for w in self.kv_w)
        self.kv_w.append(self.bf(torch.cat([lin_w(b + ".attn2.to_k"), lin_w(b + ".attn2.to_v")], 0)))
        if m._ip:
            self.kvip_w.append(self.bf(torch.cat([lin_w(b + ".attn2.processor.to_k_ip"), lin_w(b + ".attn2.processor.to_v_ip")], 0)))
        self.put_lin(b + ".attn2.out", b + ".attn2.to_out.0")
        # GEGLU: interleave [16 value rows | 16 gate rows] so a lane holds both halves of a pair
        w1 = lin_w(b + ".ff.net.0.proj")  # [8c, c]
        b1 = get(b + ".ff.net.0.proj.bias")
        half = w1.shape[0] // 2
        if m.fold_ln:   # norm3 folded in before the row interleave (a row permutation commutes with it)
            b1 = b1 + w1 @ get(b + ".norm3.bias")
            w1 = w1 * get(b + ".norm3.weight")[None, :]
        W[b + ".ff1.w"] = self.bf(torch.stack([w1[:half].reshape(half // 16, 16, -1),
                                               w1[half:].reshape(half // 16, 16, -1)], 1).reshape(2 * half, -1))
        W[b + ".ff1.b"] = torch.stack([b1[:half].reshape(half // 16, 16), b1[half:].reshape(half // 16, 16)], 1).reshape(-1).contiguous()
        if m.fold_ln:
            W[b + ".ff1.ws"] = W[b + ".ff1.w"].float().sum(1).contiguous()
        self.put_lin(b + ".ff2", b + ".ff.net.2")

    def sampler(self, name):
        self.put_conv(name, name)

    def batched(self):
        W, m = self.W, self.m
        W["kv_all.w"] = torch.cat(self.kv_w, 0).contiguous()
        if m._ip:
            W["kvip_all.w"] = torch.cat(self.kvip_w, 0).contiguous()
        m._kv_total = W["kv_all.w"].shape[0]
        W["temb_all.w"] = self.bf(torch.cat(self.temb_w, 0))
        W["temb_all.b"] = torch.cat(self.temb_b, 0).contiguous()
        m._temb_total = W["temb_all.w"].shape[0]

    def head(self):
        self.put_norm("conv_norm_out", "conv_norm_out")
        w = self.get("conv_out.weight")
        self.W["conv_out.w"] = self.bf(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1))
        self.W["conv_out.b"] = self.get("conv_out.bias").contiguous()


class _UNetPlanner:
    """The launch plan of one input geometry, written stage by stage: ``inputs``, ``time_embedding`` (with ``class_embedding`` around its
    MLP), ``added_conditions``, ``block_embeddings``, ``context_kv``, ``skip_layout``, ``walk`` (``stem``, then per layer ``resnet`` /
    ``transformer`` / ``downsample`` / ``upsample``, ``intrablock_residual`` behind the producer of each T2I-Adapter site,
    ``controlnet_residuals`` where the up path starts and ``freeu`` on every concat input) and ``head``. The attributes
    are what crosses stages: ``emb_t`` / ``emb`` / ``cls_out``, ``temb_all``, ``kv_all``, ``kvip_all``, the masks' biases, the skip layout
    (``skips``, ``ups``, ``cats``, ``cat_xc``, ``cat_hw``, ``own_skips``) and ``RES``; everything else is a local of one stage."""

    def __init__(self, model: "UNet2DConditionModel", B, H, W, L, masked=False, controlnet=False, self_mask_len=0, intrablock=0):
        self.m, self.cfg, self.lib, self.stream = model, model.cfg, model._lib, model._stream_ptr
        self.B, self.H, self.W, self.L = B, H, W, L
        self.masked, self.controlnet, self.self_mask_len = masked, controlnet, self_mask_len
        # T2I-Adapter: layer index -> residual index, for the first `intrablock` sites (intrablock_sites)
        self.intra_at = {i: n for n, i in enumerate(intrablock_sites(model._layers)[:intrablock])}
        self.pb = PlanBuilder(model, B)
        self.plan = self.pb.plan
        self.ted = self.cfg["block_out_channels"][0] * 4
        self.RES = 4 if model.resid_f32 else 2                       # bytes per element of the residual stream
        self.tmp_i = 0

    def build(self) -> _Plan:
        self.inputs()
        self.time_embedding()
        self.added_conditions()
        self.block_embeddings()
        self.context_kv()
        self.skip_layout()
        self.head(*self.walk())
        plan = self.pb.finish()
        plan.B, plan.H, plan.W, plan.L = self.B, self.H, self.W, self.L
        plan.scratch_bytes = sum(t.numel() * t.element_size() for t in plan.keep)
        return plan

    def rows(self, n, C) -> _V:
        """a persistent buffer of n rows of C 16-bit elements"""
        return _V(self.pb.persist((n, C), _lib.elem_dtype()).data_ptr(), n, C)

    def sinusoid(self, t: Tensor, t_count, n, out: _V):
        """Timesteps (flip_sin_to_cos / freq_shift of the config): t [t_count] -> out [n, out.C]"""
        self.pb.emit(self.lib.mi355x_sd_timestep_embedding,
                     (t.data_ptr(), t_count, n, out.C, 1, 1 if self.cfg["flip_sin_to_cos"] else 0, float(self.cfg["freq_shift"]), 1.0,
                      10000.0, out.p, out.ld, self.stream), "misc")

    def cast16(self, x: _V, name: str) -> _V:
        """16-bit copy of fp32 rows (operand of the down / upsampling convs in the fp32-residual mode)"""
        if x.es == 2:
            return x
        y = _V(self.pb.sc(name, 2 * x.rows * x.C), x.rows, x.C)
        self.pb.emit(self.lib.mi355x_sd_cast_rows, (x.p, x.ld, y.p, y.ld, x.rows, x.C, self.stream), "misc")
        return y

    def ln_linear(self, x: _V, nkey: str, ln: Optional[_V], wkey: str, out: _V, bias=True, flags=0):
        """LayerNorm (eps 1e-5, attention.py:318-331) into the scratch rows ``ln``, then the projection; ``ln`` None (fold_layernorm):
        the LayerNorm is folded into the projection's weights -- statistics pass + raw-row GEMM"""
        pb, lib, wp = self.pb, self.lib, self.pb.wp
        if ln is not None:
            pb.lnorm(x, nkey, ln)
            return pb.linear(ln, wkey, out, bias=bias, flags=flags)
        N, K = self.m.w[wkey + ".w"].shape
        assert K == x.C, (wkey, K, x.C)
        st = pb.sc("t_stats", 8 * x.rows)
        pb.emit(lib.mi355x_sd_row_stats, (x.p, x.rows, x.C, x.ld, 1e-5, st, self.stream), "ln")
        pb.emit(lib.mi355x_sd_linear_ln, (x.p, x.ld, st, wp(wkey + ".w"), wp(wkey + ".ws"), out.p, out.ld, x.rows, N, K,
                                          wp(wkey + ".b"), flags, *self.m._gemm_ws, self.stream), "gemm", 2.0 * x.rows * N * K,
                f"{x.rows}x{N}x{K}" + ("g" if flags & GEGLU else ""))

    def attention(self, q: _V, k: _V, v: _V, out: _V, heads, sq, skv, bias=None, accum: Optional[float] = None, log2=False):
        sdpa, lib = self.pb.sdpa, self.lib
        if log2 and bias is not None:
            # q already carries head_dim^-0.5 * log2(e) (folded into to_q at load) but the masked kernel exponentiates
            # exp2((q.k + bias / scale) * scale * log2(e)): scale = ln 2 makes that exp2(q.k + bias * log2(e)) -- the same softmax
            assert accum is None
            sdpa(q, k, v, out, heads, sq, skv, bias, (skv, 0, 0), math.log(2.0), suffix="m")
        elif log2:
            assert accum is None and q.C // heads == 64
            sdpa(q, k, v, out, heads, sq, skv, scale=1.0, fn=lib.mi355x_sd_sdpa_ex, tail=(SDPA_LOG2,))
        elif accum is None:
            # bias: additive encoder mask [B, skv] broadcast over heads and queries (unet_2d_condition.py:921-927)
            sdpa(q, k, v, out, heads, sq, skv, bias, (skv if bias else 0, 0, 0))
        else:   # out += accum * attention (the image-token half of IPAdapterAttnProcessor)
            sdpa(q, k, v, out, heads, sq, skv, bias, (skv if bias else 0, 0, 0), fn=lib.mi355x_sd_sdpa_accum, tail=(float(accum),),
                 suffix="+")

    # ---- stages ----
    def inputs(self):
        """static buffers, staged by __call__"""
        plan, persist, cfg, B, L = self.plan, self.pb.persist, self.cfg, self.B, self.L
        plan.sample = persist((B, cfg["in_channels"], self.H, self.W), torch.float32)
        plan.t = persist((1,), torch.float32)
        plan.in_scale = persist((1,), torch.float32)
        plan.in_scale.fill_(1.0)
        plan.enc = persist((B * L, cfg["cross_attention_dim"][0]), _lib.elem_dtype())
        plan.out = persist((B, cfg["out_channels"], self.H, self.W), torch.float32)
        plan.enc_bias = persist((B, L), torch.float32) if self.masked else None
        self.enc_bias = plan.enc_bias.data_ptr() if self.masked else None
        # `attention_mask`: a key mask over the LATENT tokens, added to every self-attention (unet_2d_condition.py:916-923 ->
        # BasicTransformerBlock.attn1, attention.py:417-423)
        plan.self_bias = persist((B, self.self_mask_len), torch.float32) if self.self_mask_len else None
        self.self_bias = plan.self_bias.data_ptr() if self.self_mask_len else None

    def time_embedding(self):
        """sinusoid, cond_proj, the time MLP (unet_2d_condition.py:933-951), with the class embedding's two halves around the MLP"""
        plan, cfg, B, ted, linear = self.plan, self.cfg, self.B, self.ted, self.pb.linear
        t0_t = self.pb.persist((B, cfg["block_out_channels"][0]), _lib.elem_dtype())
        t0 = _V.of(t0_t)
        self.sinusoid(plan.t, 1, B, t0)
        e1 = self.rows(B, ted)
        ted_b = ted * (2 if cfg["class_embeddings_concat"] else 1)
        emb_t = self.pb.persist((B, ted_b), _lib.elem_dtype())
        plan.emb_tensors = dict(t0=t0_t, emb=emb_t)
        self.emb_t = _V.of(emb_t)
        self.emb = self.emb_t.cols(0, ted)                 # the time-embedding half (all of it without concat)
        self.cls_out = self.emb_t.cols(ted, ted) if ted_b > ted else None     # where the class embedding goes when concatenated
        plan.class_in = None
        pre_cls = self.class_embedding(before_mlp=True)
        plan.tcond = None
        if cfg["time_cond_proj_dim"] is not None:   # t_emb += cond_proj(timestep_cond) (embeddings.py:284-285; zeros when not given)
            plan.tcond = self.pb.persist((B, cfg["time_cond_proj_dim"]), _lib.elem_dtype())
            plan.tcond.zero_()
            linear(_V.of(plan.tcond), "time_embedding.cond_proj", t0, bias=False, R=t0)
        linear(t0, "time_embedding.linear_1", e1, flags=SILU)
        linear(e1, "time_embedding.linear_2", self.emb, R=pre_cls)
        self.class_embedding(before_mlp=False)

    def class_embedding(self, before_mlp: bool) -> Optional[_V]:
        """class embedding (unet_2d_condition.py:953-975): emb + class_emb, or [emb | class_emb] when class_embeddings_concat. The add
        is the residual input of a GEMM epilogue, the concat is a GEMM / gather writing the upper columns. ``before_mlp``: a gathered /
        identity embedding exists before the time MLP and is returned, to be added as the MLP's residual; the computed kinds follow it."""
        plan, pb, cfg, B, ted, ck, cls_out = self.plan, self.pb, self.cfg, self.B, self.ted, self.m._class_kind, self.cls_out
        if before_mlp and ck == "embedding":
            plan.class_in = pb.persist((B,), torch.int32)
            dst = cls_out or self.rows(B, ted)
            pb.emit(self.lib.mi355x_sd_embed_tokens, (plan.class_in.data_ptr(), B, 1, pb.wp("class_embedding.table"), None, ted, dst.p,
                                                      dst.ld, self.stream), "misc")
            return None if cls_out else dst
        if before_mlp and ck == "identity":
            plan.class_in = pb.persist((B, ted), _lib.elem_dtype())
            src = _V.of(plan.class_in)
            if not cls_out:
                return src
            pb.emit(self.lib.mi355x_sd_copy_rows, (src.p, src.ld, cls_out.p, cls_out.ld, B, ted, self.stream), "misc")
        if before_mlp or ck not in ("timestep", "projection", "simple_projection"):
            return None
        if ck == "timestep":   # class_labels -> sinusoid (time_proj) -> TimestepEmbedding
            plan.class_in = pb.persist((B,), torch.float32)
            cin = self.rows(B, cfg["block_out_channels"][0])
            self.sinusoid(plan.class_in, B, B, cin)
        else:
            plan.class_in = pb.persist((B, cfg["projection_class_embeddings_input_dim"]), _lib.elem_dtype())
            cin = _V.of(plan.class_in)
        dst, res = (cls_out, None) if cls_out else (self.emb, self.emb)
        if ck == "simple_projection":
            pb.linear(cin, "class_embedding", dst, R=res)
        else:
            c1 = self.rows(B, ted)
            pb.linear(cin, "class_embedding.linear_1", c1, flags=SILU)
            pb.linear(c1, "class_embedding.linear_2", dst, R=res)
        return None

    def added_conditions(self):
        """text_time (unet_2d_condition.py:991-1010): emb += MLP([text_embeds | sinusoid(time_ids)]); _finish_add_embedding inserts the
        sinusoid's launch once the first call shows the widths of text_embeds / time_ids"""
        plan, pb, cfg, B = self.plan, self.pb, self.cfg, self.B
        plan.add_in = plan.time_ids = None
        if cfg["addition_embed_type"] != "text_time":
            return
        plan._pdim, plan._atd = cfg["projection_class_embeddings_input_dim"], cfg["addition_time_embed_dim"]
        plan.add_in = pb.persist((B, plan._pdim), _lib.elem_dtype())
        plan.text_dim = None
        a1 = self.rows(B, self.ted)
        plan._add_emit_index = len(pb.prog)
        pb.linear(_V.of(plan.add_in), "add_embedding.linear_1", a1, flags=SILU)
        pb.linear(a1, "add_embedding.linear_2", self.emb, R=self.emb)

    def block_embeddings(self):
        """SiLU(emb) -> every resnet's time_emb_proj in one GEMM"""
        pb, B, m, emb_t = self.pb, self.B, self.m, self.emb_t
        semb = self.rows(B, emb_t.C)
        pb.emit(self.lib.mi355x_sd_silu, (emb_t.p, semb.p, B * emb_t.C, 0, 0, self.stream), "misc")
        self.temb_all = pb.persist((B, m._temb_total), torch.float32)
        pb.linear(semb, "temb_all", _V(self.temb_all.data_ptr(), B, m._temb_total), flags=OUT_F32)
        self.plan.emb_tensors["temb_all"] = self.temb_all

    def context_kv(self):
        """every block's cross-attention K/V projection of encoder_hidden_states in one GEMM (attention_processor.py:711-712).
        IP-Adapter (unet_2d_condition.py:1054-1061): image_embeds -> ImageProjection (Linear, view [B*T, Dx], LayerNorm) -> the image
        tokens' K/V for every cross-attention in one GEMM. The reference appends the tokens to encoder_hidden_states and each
        IPAdapterAttnProcessor splits them off again; here they never join the text rows."""
        plan, pb, cfg, B, m = self.plan, self.pb, self.cfg, self.B, self.m
        self.kv_all = self.rows(B * self.L, m._kv_total)
        pb.linear(_V.of(plan.enc), "kv_all", self.kv_all, bias=False)
        plan.image_embeds = self.kvip_all = None
        if not m._ip:
            return
        dx, T = cfg["cross_attention_dim"][0], cfg["ip_adapter_num_tokens"]
        plan.image_embeds = pb.persist((B, cfg["encoder_hid_dim"]), _lib.elem_dtype())
        raw = self.rows(B, T * dx)
        pb.linear(_V.of(plan.image_embeds), "encoder_hid_proj.image_embeds", raw)
        tok = self.rows(B * T, dx)
        pb.lnorm(_V(raw.p, B * T, dx), "encoder_hid_proj.norm", tok)
        self.kvip_all = self.rows(B * T, m._kv_total)
        pb.linear(tok, "kvip_all", self.kvip_all, bias=False)

    def skip_layout(self):
        """the pre-walk: every skip connection is produced inside the buffer its up-block consumer reads (concat by construction); a
        layer list without an up path (ControlNetModel) gets buffers of the skips' own"""
        B, RES, S = self.B, self.RES, self.m._layers
        self.skips: List[Tuple[int, int, int]] = []  # (C, h, w) in production order
        h, w_, c_cur = self.H, self.W, self.cfg["block_out_channels"][0]
        for d in S:
            if d[0] == "resnet":
                c_cur = d[3]
            elif d[0] == "down":
                h, w_ = (h + 2 - 3) // 2 + 1, (w_ + 2 - 3) // 2 + 1
            elif d[0] == "skip":
                self.skips.append((c_cur, h, w_))
            elif d[0] == "cat":
                break
        self.ups = [d for d in S if d[0] == "resnet" and d[1].startswith("up_blocks.")]
        assert not self.ups or len(self.ups) == len(self.skips)
        self.own_skips = None if self.ups else [self.rows(B * hs * ws_, cs) for cs, hs, ws_ in self.skips]
        self.cats: List[_V] = []
        self.cat_xc: List[int] = []
        self.cat_hw: List[Tuple[int, int]] = []
        for u, d in enumerate(self.ups):  # up resnet u consumes skip n-1-u
            cs, hs, ws_ = self.skips[len(self.skips) - 1 - u]
            t = self.pb.persist((B * hs * ws_, d[2]), torch.float32 if RES == 4 else _lib.elem_dtype())
            self.cats.append(_V(t.data_ptr(), B * hs * ws_, d[2], es=RES))
            self.cat_xc.append(d[2] - cs)
            self.cat_hw.append((hs, ws_))

    def skip_slot(self, k: int) -> _V:  # where skip k is produced
        if self.own_skips is not None:
            return self.own_skips[k]
        u = len(self.skips) - 1 - k
        return self.cats[u].cols(self.cat_xc[u], self.cats[u].C - self.cat_xc[u])

    def x_slot(self, u: int) -> _V:
        return self.cats[u].cols(0, self.cat_xc[u])

    def tmp(self, rows, c) -> _V:
        self.tmp_i ^= 1
        return _V(self.pb.sc(f"x{self.tmp_i}", self.RES * rows * c), rows, c, es=self.RES)

    def resnet(self, name, x: _V, h, w_, cout, scale, out: _V):
        pb, m, RES, sc, eps = self.pb, self.m, self.RES, self.pb.sc, float(self.cfg["norm_eps"])
        hw = h * w_
        rows = self.B * hw
        need_short = x.C != cout
        x16 = _V(sc("x16", 2 * rows * x.C), rows, x.C) if (need_short and x.es == 4) else None
        g1 = pb.gnorm(x, hw, name + ".norm1", eps, True, raw16=x16)
        h1 = _V(sc("h1", RES * rows * cout), rows, cout, es=RES)   # fp32 mode: GroupNorm 2 reads the unrounded conv1 output
        rb = self.temb_all.data_ptr() + 4 * m._temb_off[name]
        pb.conv3(g1, h, w_, name + ".conv1", h1, rowbias=rb, ld_rb=m._temb_total)
        g2 = pb.gnorm(h1, hw, name + ".norm2", eps, True)
        if need_short:
            short = _V(sc("short", RES * rows * cout), rows, cout, es=RES)
            pb.linear(x16 if x16 is not None else x, name + ".conv_shortcut", short)
        else:
            short = x
        pb.conv3(g2, h, w_, name + ".conv2", out, R=short, out_scale=1.0 / scale)

    def transformer(self, name, x: _V, h, w_, heads, layers, out: _V):
        pb, m, RES, sc, linear, ln_linear = self.pb, self.m, self.RES, self.pb.sc, self.pb.linear, self.ln_linear
        hw = h * w_
        rows = self.B * hw
        c = x.C
        g = pb.gnorm(x, hw, name + ".norm", 1e-6, False)
        hid = _V(sc("t_h", RES * rows * c), rows, c, es=RES)
        hid16 = _V(sc("t_h16", 2 * rows * c), rows, c) if RES == 4 else hid   # proj_out's operand: the last FF2 writes it
        linear(g, name + ".proj_in", hid)
        ln = None if m.fold_ln else _V(sc("t_ln", 2 * rows * c), rows, c)
        qkv = _V(sc("t_qkv", 2 * rows * 3 * c), rows, 3 * c)
        ao = _V(sc("t_ao", 2 * rows * c), rows, c)
        ff = _V(sc("t_ff", 2 * rows * 4 * c), rows, 4 * c)
        for l in range(layers):
            b = f"{name}.transformer_blocks.{l}"
            q2 = _V(qkv.p, rows, c)
            ln_linear(hid, b + ".norm1", ln, b + ".attn1.qkv", qkv, bias=False)
            if self.self_bias is not None and hw != self.self_mask_len:
                # the reference pads a mask of the wrong length by target_length zeros (Attention.prepare_attention_mask,
                # attention_processor.py:616-622) and the add onto the [.., hw, hw] scores then fails on the shapes
                raise ValueError(f"attention_mask has {self.self_mask_len} key tokens but {b}.attn1 attends over {hw} latent tokens "
                                 "(the mask must match the token count of every attention level)")
            self.attention(qkv.cols(0, c), qkv.cols(c, c), qkv.cols(2 * c, c), ao, heads, hw, hw, bias=self.self_bias,
                           log2=b in m._log2_blocks)
            linear(ao, b + ".attn1.out", hid, R=hid)
            ln_linear(hid, b + ".norm2", ln, b + ".attn2.q", q2, bias=False)
            ko = m._kv_off[b]
            self.attention(q2, self.kv_all.cols(ko, c), self.kv_all.cols(ko + c, c), ao, heads, hw, self.L, bias=self.enc_bias)
            if self.kvip_all is not None and m.ip_adapter_scale != 0.0:
                self.attention(q2, self.kvip_all.cols(ko, c), self.kvip_all.cols(ko + c, c), ao, heads, hw,
                               self.cfg["ip_adapter_num_tokens"], accum=m.ip_adapter_scale)
            linear(ao, b + ".attn2.out", hid, R=hid)
            ln_linear(hid, b + ".norm3", ln, b + ".ff1", ff, flags=GEGLU)
            linear(ff, b + ".ff2", hid16 if l == layers - 1 else hid, R=hid)
        linear(hid16, name + ".proj_out", out, R=x)

    def downsample(self, name, x: _V, h, w_, out: _V):
        self.pb.conv3(self.cast16(x, "xc16"), h, w_, name, out, stride=2)

    def upsample(self, name, x: _V, h, w_, ht, wt, out: _V):
        """to (ht, wt), the size of the skip the next resnet concatenates with"""
        pb, B = self.pb, self.B
        src = self.cast16(x, "xc16")
        if (ht, wt) == (2 * h, 2 * w_):
            return pb.conv3(src, h, w_, name, out, up=1)     # nearest x2 folded into the conv's gather
        # `forward_upsample_size` (unet_2d_condition.py:900-906, :1165-1169; Upsample2D interpolates to the skip's size):
        # latents that are not multiples of 2^(levels - 1) leave a skip of odd size 2h - 1, and nearest interpolation
        # from h to 2h - 1 reads source row y >> 1 like the x2 form, cropped. The crop moves the zero padding of the
        # conv, so the upsampled tensor is materialised here (strided row copies: one per source row and parity --
        # many small launches, on this rare path only) and a plain 3x3 conv follows.
        assert ht in (2 * h - 1, 2 * h) and wt in (2 * w_ - 1, 2 * w_), (h, w_, ht, wt)
        C_ = src.C
        upb = _V(pb.sc("upx", 2 * B * ht * wt * C_), B * ht * wt, C_)
        for b in range(B):
            for i_ in range(h):
                for y in (2 * i_, 2 * i_ + 1)[:ht - 2 * i_]:   # (a skip of odd height 2h - 1 has no row 2h - 1)
                    for dx in (0, 1):
                        pb.emit(self.lib.mi355x_sd_copy_rows, (src.p + 2 * ((b * h + i_) * w_) * src.ld, src.ld,
                                                               upb.p + 2 * ((b * ht + y) * wt + dx) * C_, 2 * C_, (wt - dx + 1) // 2, C_,
                                                               self.stream), "misc")
        pb.conv3(upb, ht, wt, name, out)

    def controlnet_residuals(self, mid: _V, h, w_):
        """ControlNet residuals (unet_2d_condition.py:1121-1132, 1151-1155): every skip tensor and the mid output get their residual
        once the down path and the mid block have consumed the originals"""
        if not self.controlnet:
            return
        plan, add = self.plan, self.add_nchw
        plan.ctrl_down = [add(self.skip_slot(k), *s) for k, s in enumerate(self.skips)]
        plan.ctrl_mid = add(mid, mid.C, h, w_)

    def add_nchw(self, dst: _V, c, hs, ws_) -> Tensor:
        """dst += a residual the caller hands over as fp32 NCHW, in place; returns the persistent buffer ``stage_inputs`` fills"""
        pb, B = self.pb, self.B
        r = pb.persist((B, c, hs, ws_), torch.float32)
        if dst.es == 2:
            pb.emit(self.lib.mi355x_sd_add_nchw, (dst.p, dst.ld, r.data_ptr(), B, c, hs * ws_, self.stream), "misc")
        else:
            pb.emit(self.lib.mi355x_sd_add_nchw_ex, (dst.p, dst.ld, r.data_ptr(), B, c, hs * ws_, 1, self.stream), "misc")
        return r

    def intrablock_residual(self, i: int, cur: _V, h, w_):
        """T2I-Adapter residuals (``down_intrablock_additional_residuals``, unet_2d_condition.py:1096-1119, 1146-1152;
        unet_2d_blocks.py:1211-1213): layer ``i`` is a site -- the last resnet / attention pair of a CrossAttnDownBlock2D, the end of a
        DownBlock2D (its downsampler if it has one), the mid block -- so its output gets its residual in place, directly behind the
        launch that produced it and before anything reads it: the tensor is a skip and the next layer's input at once"""
        if i in self.intra_at:
            assert self.intra_at[i] == len(self.plan.intra)
            self.plan.intra.append(self.add_nchw(cur, cur.C, h, w_))

    def freeu(self, u: int):
        """FreeU (apply_freeu, unet_2d_blocks.py:2329-2351, 2478-2500): the concat input of up resnet ``u``, in place, before its first
        GroupNorm -- backbone half * b, skip planes Fourier-filtered with scale s, for the resnets of up blocks 0 (b1, s1) and 1 (b2, s2)"""
        fu = self.m.freeu
        if fu is None:
            return
        name = self.ups[u][1]
        i = 0 if name.startswith("up_blocks.0.") else 1 if name.startswith("up_blocks.1.") else None
        if i is None:
            return
        s, b = fu[i], fu[2 + i]
        cat, cx, (h, w_) = self.cats[u], self.cat_xc[u], self.cat_hw[u]
        cs = cat.C - cx
        ws = self.pb.sc("freeu_ws", 4 * self.lib.mi355x_sd_freeu_workspace_floats(self.B, h, w_, cs))
        self.pb.emit(self.lib.mi355x_sd_freeu, (cat.p, cat.ld, self.B, h, w_, cx, cs, b, s, 1 if cat.es == 4 else 0, ws, self.stream),
                     "freeu", 0.0, f"{self.B}x{h}x{w_}x{cx}+{cs}")

    def stem(self) -> _V:
        """conv_in writes skip 0"""
        plan, pb, cfg = self.plan, self.pb, self.cfg
        cur = self.skip_slot(0)
        args = (plan.sample.data_ptr(), plan.in_scale.data_ptr(), pb.wp("conv_in.w"), pb.wp("conv_in.b"), cur.p, self.B,
                cfg["in_channels"], self.H, self.W, cfg["block_out_channels"][0], cur.ld)
        if cur.es == 2:
            pb.emit(self.lib.mi355x_sd_conv_in3x3, args + (self.stream,), "misc")
        else:
            pb.emit(self.lib.mi355x_sd_conv_in3x3_ex, args + (1, self.stream), "misc")
        return cur

    def walk(self):
        """the loop over the layer list that picks each layer's destination; returns the last output and its size"""
        S, B = self.m._layers, self.B
        h, w_ = self.H, self.W
        k, u = 1, 0          # next skip index to produce (S[0] is the conv_in skip), next up resnet index
        self.plan.intra = []
        cur = self.stem()
        for i in range(1, len(S)):
            d = S[i]
            nxt = S[i + 1][0] if i + 1 < len(S) else "end"
            if d[0] in ("resnet", "attn"):
                cout = d[3] if d[0] == "resnet" else d[2]
                if nxt == "skip":
                    dst = self.skip_slot(k)
                elif nxt == "cat":
                    dst = self.x_slot(u)
                else:  # followed by a transformer / the mid resnet / an upsampler / the head
                    dst = self.tmp(B * h * w_, cout)
                if d[0] == "resnet":
                    self.resnet(d[1], cur, h, w_, cout, d[4], dst)
                else:
                    self.transformer(d[1], cur, h, w_, d[3], d[4], dst)
                cur = dst
                self.intrablock_residual(i, cur, h, w_)
            elif d[0] == "skip":
                k += 1
            elif d[0] == "down":
                dst = self.skip_slot(k)
                self.downsample(d[1], cur, h, w_, dst)
                h, w_ = (h + 2 - 3) // 2 + 1, (w_ + 2 - 3) // 2 + 1
                cur = dst
                self.intrablock_residual(i, cur, h, w_)
            elif d[0] == "cat":
                if u == 0:
                    self.controlnet_residuals(cur, h, w_)
                self.freeu(u)
                cur = self.cats[u]
                u += 1
            elif d[0] == "up":
                dst = self.x_slot(u)
                self.upsample(d[1], cur, h, w_, *self.cat_hw[u], dst)
                h, w_ = self.cat_hw[u]
                cur = dst
        assert k == len(self.skips) and u == len(self.ups) and (not self.ups or (h, w_) == (self.H, self.W))
        return cur, h, w_

    def head(self, x: _V, h, w_):
        """conv_norm_out + conv_out (unet_2d_condition.py:1193-1196)"""
        pb, cfg = self.pb, self.cfg
        g = pb.gnorm(x, h * w_, "conv_norm_out", float(cfg["norm_eps"]), True)
        pb.emit(self.lib.mi355x_sd_conv_out3x3, (g.p, g.ld, pb.wp("conv_out.w"), pb.wp("conv_out.b"), self.plan.out.data_ptr(), self.B,
                                                 g.C, h, w_, cfg["out_channels"], self.stream), "misc")


class UNet2DConditionOutput(SimpleNamespace):
    """``.sample`` holder, mirroring unet_2d_condition.py:61-72."""


class UNet2DConditionModel(DeviceProgram, PretrainedMixin):
    _param_shapes = staticmethod(unet_param_shapes)

    def __init__(self, config: Mapping, params: Mapping[str, Tensor], device="cuda", use_graph: bool = True,
                 profile: bool = False, fold_layernorm: Optional[bool] = None, residual_dtype: Optional[str] = None,
                 fold_softmax_scale: Optional[bool] = None):
        """The model needs the built HIP library and a GPU, and raises otherwise (there is no CPU fallback)."""
        self._init_backend(device, use_graph, profile)
        # fold_layernorm: LayerNorms of the transformer blocks folded into their consuming projections (row statistics
        # pass + mi355x_sd_linear_ln on the raw rows). Off by default: on MI355X it removes 2.3 ms of LayerNorm
        # traffic per SDXL step but the GEMMs then multiply the raw residual stream instead of O(1) normalised
        # activations and run 6-12 % slower (operand-dependent MFMA power), a wash end to end
        # (profiles/r01_lnfold_ab.txt; round 6, on today's kernels: 58.0 vs 56.3 ms per step -- the folded QKV / FF1 launches also lose
        # the four-wave tile, which has no row-statistics epilogue: profiles/r06_s40_lnfold_ab.txt). MI355X_SD_LNFOLD=1 or
        # fold_layernorm=True turns it on.
        self.fold_ln = (os.environ.get("MI355X_SD_LNFOLD") is not None) if fold_layernorm is None else bool(fold_layernorm)
        # residual_dtype="fp32" (or MI355X_SD_RESID=fp32): the residual stream -- resnet outputs, the transformer blocks' hidden
        # state, every skip / concat slot -- is stored in fp32; 16-bit values exist only as MFMA operands (the outputs of
        # GroupNorm / LayerNorm / GEGLU / attention, which feed exactly one contraction each). Each branch then rounds once
        # instead of the stream re-rounding after every one of its ~50-200 sequential adds.
        # fold_softmax_scale (default on; MI355X_SD_FOLD_SCALE=0 turns it off): head_dim^-0.5 * log2(e) is multiplied into the self-attention to_q weights
        # at load (fp32, before the one rounding to 16 bits), so q.k IS the base-2 exponent of the softmax and the attention
        # kernel runs its MI355X_SD_SDPA_LOG2 form (no multiply-add per score). Same function, slightly different rounding of
        # the to_q weights (they are rounded after the scaling instead of before); self-attention with head_dim 64 only.
        self.fold_scale = (os.environ.get("MI355X_SD_FOLD_SCALE", "1") == "1") if fold_softmax_scale is None else bool(fold_softmax_scale)
        rd = os.environ.get("MI355X_SD_RESID", "") if residual_dtype is None else residual_dtype
        if rd not in ("", None, "fp32", "16"):
            raise ValueError(f"residual_dtype must be None | '16' | 'fp32', got {rd!r}")
        self.resid_f32 = rd == "fp32"
        if self.resid_f32 and (self.fold_ln or self._encoder_only):
            raise NotImplementedError("residual_dtype='fp32' with fold_layernorm / ControlNetModel")
        self.cfg = normalize_config(config)
        # .config shows the constructor arguments as given (register_to_config), not the per-block expansion
        pub = dict(UNET_DEFAULTS)
        pub.update({k: v for k, v in config.items() if not k.startswith("_")})
        self.config = SimpleNamespace(**pub)
        if self.cfg["addition_embed_type"] == "text_time":
            # StableDiffusionXLPipeline._get_add_time_ids (pipeline_stable_diffusion_xl.py:603-619) sizes its check from
            # `unet.add_embedding.linear_1.in_features`: the one sub-layer attribute a pipeline reads off the UNet
            pdim = self.cfg["projection_class_embeddings_input_dim"]
            self.add_embedding = SimpleNamespace(linear_1=SimpleNamespace(in_features=pdim, out_features=self.cfg["block_out_channels"][0] * 4))
        ct = self.cfg["class_embed_type"]
        self._class_kind = "embedding" if (ct is None and self.cfg["num_class_embeds"] is not None) else ct
        self._ip = self.cfg["encoder_hid_dim_type"] == "ip_image_proj"
        self.ip_adapter_scale = 1.0
        self.freeu: Optional[Tuple[float, float, float, float]] = None   # (s1, s2, b1, b2) while FreeU is on
        self._layers = _structure(self.cfg, self._encoder_only)
        self._Weights(self, params).load()

    _encoder_only = False   # ControlNetModel: the layer list stops after the mid block
    _Weights, _Planner = _UNetWeights, _UNetPlanner   # ControlNetModel overrides stages of both

    def _shapes(self) -> Dict[str, tuple]:
        return unet_param_shapes(self.cfg)

    # ------------------------------------------------------------------ execution
    def _finish_add_embedding(self, plan: _Plan, text_dim: int, n_ids: int) -> None:
        """text_time (unet_2d_condition.py:991-1010): add_in = [text_embeds | sinusoid(time_ids.flatten())]."""
        cfg, lib = self.cfg, self._lib
        if text_dim + n_ids * plan._atd != plan._pdim:
            raise ValueError(f"text_embeds ({text_dim}) + time_ids ({n_ids} x {plan._atd}) != "
                             f"projection_class_embeddings_input_dim ({plan._pdim})")
        B = plan.B
        plan.text_dim, plan.n_ids = text_dim, n_ids
        plan.time_ids = torch.empty((B * n_ids,), device=self.device, dtype=torch.float32)
        plan.keep.append(plan.time_ids)
        op = (lib.mi355x_sd_timestep_embedding,
              (plan.time_ids.data_ptr(), B * n_ids, B * n_ids, plan._atd, n_ids, 1 if cfg["flip_sin_to_cos"] else 0,
               float(cfg["freq_shift"]), 1.0, 10000.0, plan.add_in.data_ptr() + 2 * text_dim, plan._pdim,
               self._stream_ptr), "misc", 0.0)
        plan.prog.insert(plan._add_emit_index, op)

    def set_ip_adapter_scale(self, scale: float) -> None:
        """weight of the image prompt in every cross-attention (IPAdapterAttnProcessor.scale; the pipelines'
        ``set_ip_adapter_scale``, loaders/ip_adapter.py). The scale is a launch constant: plans are per scale; 0 drops the
        image-token attention launches altogether."""
        if not self._ip:
            raise ValueError("this UNet has no IP-Adapter (config encoder_hid_dim_type != 'ip_image_proj')")
        self.ip_adapter_scale = float(scale)

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float) -> None:
        """FreeU (https://arxiv.org/abs/2309.11497; unet_2d_condition.py:777-801): in the first two up blocks the first half of the
        backbone channels is multiplied by b1 / b2 and the skip features are Fourier-filtered with scale s1 / s2 before every resnet.
        The four values are launch constants: plans are per setting."""
        vals = tuple(float(v) for v in (s1, s2, b1, b2))
        if not all(math.isfinite(v) for v in vals):
            raise ValueError(f"enable_freeu: s1, s2, b1, b2 must be finite, got {vals}")
        self.freeu = vals

    def disable_freeu(self) -> None:
        """unet_2d_condition.py:803-808"""
        self.freeu = None

    def _get_plan(self, B, H, W, L, masked: bool = False, controlnet: bool = False, self_mask_len: int = 0,
                  intrablock: int = 0) -> _Plan:
        """``intrablock``: how many T2I-Adapter residuals the plan adds (the first so many of ``intrablock_shapes``); none leaves the
        key and the plan what they are without the argument"""
        if masked and self._ip:
            raise NotImplementedError("encoder_attention_mask together with IP-Adapter image tokens")
        key = (B, H, W, L, masked, controlnet, self.ip_adapter_scale, self_mask_len, self.freeu) + ((intrablock,) if intrablock else ())
        return self.plan_for(key, lambda: self._Planner(self, B, H, W, L, masked, controlnet, self_mask_len, intrablock).build())

    def intrablock_shapes(self, B, H, W) -> List[Tuple[int, int, int, int]]:
        """shape of the residual each T2I-Adapter site takes for a [B, C, H, W] sample, in the order of
        ``down_intrablock_additional_residuals``: one per down block, then the mid block's"""
        out, h, w_, c = [], H, W, self.cfg["block_out_channels"][0]
        sites = intrablock_sites(self._layers)
        for i, d in enumerate(self._layers):
            if d[0] == "resnet":
                c = d[3]
            elif d[0] == "down":
                h, w_ = (h + 2 - 3) // 2 + 1, (w_ + 2 - 3) // 2 + 1
            if i in sites:
                out.append((B, c, h, w_))
        return out

    def _intrablock_count(self, residuals, sample_shape, deprecated: bool) -> int:
        """how many of ``residuals`` the forward adds, by the reference's rules (unet_2d_condition.py:1096-1119, 1146-1152): one per
        down block while the list lasts, then the next one after the mid block if it has the mid output's shape; what is left over is
        ignored. A down block's residual of another shape is an error (the reference's add fails on it)."""
        B, _, H, W = sample_shape
        shapes = self.intrablock_shapes(B, H, W)
        n = min(len(residuals), len(shapes) - 1)
        for k in range(n):
            if tuple(residuals[k].shape) != shapes[k]:
                if deprecated:
                    raise NotImplementedError(
                        "`down_block_additional_residuals` without `mid_block_additional_residual` is read as T2I-Adapter residuals "
                        f"(the deprecated form of `down_intrablock_additional_residuals`), and residual {k} of shape "
                        f"{tuple(residuals[k].shape)} is not down block {k}'s {shapes[k]}; ControlNet residuals need both "
                        "`down_block_additional_residuals` and `mid_block_additional_residual`")
                raise ValueError(f"down_intrablock_additional_residuals[{k}] of shape {tuple(residuals[k].shape)}, expected "
                                 f"{shapes[k]} (the output of down block {k})")
        if len(residuals) > n and tuple(residuals[n].shape) == shapes[-1]:
            n += 1
        return n

    def stage_inputs(self, plan: _Plan, sample, timestep, encoder_hidden_states, added_cond_kwargs=None,
                     in_scale: Optional[float] = None, encoder_attention_mask=None,
                     down_block_additional_residuals=None, mid_block_additional_residual=None, class_labels=None,
                     timestep_cond=None, attention_mask=None, down_intrablock_additional_residuals=None) -> None:
        cfg = self.cfg
        intra = getattr(plan, "intra", None) or []
        if intra:
            given = down_intrablock_additional_residuals
            if given is None or len(given) < len(intra):
                raise ValueError(f"this plan adds {len(intra)} down_intrablock_additional_residuals, got "
                                 f"{0 if given is None else len(given)}")
            for k, (dst, r) in enumerate(zip(intra, given)):   # (surplus residuals are ignored, like the reference's pop)
                if tuple(r.shape) != tuple(dst.shape):
                    raise ValueError(f"down_intrablock_additional_residuals[{k}] of shape {tuple(r.shape)}, expected {tuple(dst.shape)}")
                dst.copy_(r, non_blocking=True)
        if getattr(plan, "self_bias", None) is not None:
            # (1 - mask) * -10000 as an additive bias on the self-attention scores (unet_2d_condition.py:916-923)
            plan.self_bias.copy_((1.0 - attention_mask.to(torch.float32)) * -10000.0, non_blocking=True)
        if plan.tcond is not None:
            if timestep_cond is None:
                plan.tcond.zero_()   # cond_proj has no bias: a zero condition adds nothing, like the reference's `condition is None`
            else:
                if tuple(timestep_cond.shape) != tuple(plan.tcond.shape):
                    raise ValueError(f"timestep_cond of shape {tuple(timestep_cond.shape)}, expected {tuple(plan.tcond.shape)}")
                plan.tcond.copy_(timestep_cond.to(plan.tcond.dtype), non_blocking=True)
        elif timestep_cond is not None:
            raise ValueError("timestep_cond was passed but the model has no `time_cond_proj_dim`")
        if plan.class_in is not None:
            if class_labels is None:
                raise ValueError("class_labels should be provided when num_class_embeds > 0")
            cl = class_labels if torch.is_tensor(class_labels) else torch.as_tensor(class_labels)
            if plan.class_in.dim() == 1:   # embedding ids / timestep-like labels: one per batch row
                cl = cl.reshape(-1)
                cl = cl.expand(plan.B) if cl.numel() == 1 else cl
            if tuple(cl.shape) != tuple(plan.class_in.shape):
                raise ValueError(f"class_labels of shape {tuple(class_labels.shape)}, expected {tuple(plan.class_in.shape)}")
            if self._class_kind == "embedding" and not cl.is_cuda and cl.numel() and not (
                    0 <= int(cl.min()) and int(cl.max()) < cfg["num_class_embeds"]):
                # nn.Embedding's range check, where it costs nothing (host labels; a device tensor is not read back: the gather
                # kernel trusts its indices, like the reference's GPU kernel)
                raise IndexError(f"class_labels must lie in [0, {cfg['num_class_embeds']}), got {cl.tolist()}")
            plan.class_in.copy_(cl.to(plan.class_in.dtype), non_blocking=True)
        if getattr(plan, "ctrl_down", None) is not None:
            if len(down_block_additional_residuals) != len(plan.ctrl_down):
                raise ValueError(f"expected {len(plan.ctrl_down)} down_block_additional_residuals, got "
                                 f"{len(down_block_additional_residuals)}")
            for dst, r in zip(plan.ctrl_down + [plan.ctrl_mid],
                              list(down_block_additional_residuals) + [mid_block_additional_residual]):
                if tuple(r.shape) != tuple(dst.shape):
                    raise ValueError(f"ControlNet residual of shape {tuple(r.shape)}, expected {tuple(dst.shape)}")
                dst.copy_(r, non_blocking=True)
        if plan.enc_bias is not None:
            # (1 - mask) * -10000 as an additive bias (unet_2d_condition.py:921-927)
            plan.enc_bias.copy_((1.0 - encoder_attention_mask.to(torch.float32)) * -10000.0, non_blocking=True)
        if torch.is_tensor(timestep):
            tv = timestep.reshape(-1)
            if tv.numel() > 1 and (tv.numel() != plan.B or not bool((tv == tv[0]).all())):
                # the program reads ONE timestep (what the pipelines pass, pipeline_stable_diffusion.py:866-879); the reference would
                # broadcast a [B] tensor per sample (unet_2d_condition.py:946)
                raise ValueError("timestep: per-sample timesteps are not implemented (pass one value, or B equal values)")
            plan.t.copy_(tv[:1].to(torch.float32), non_blocking=True)
        else:
            plan.t.fill_(float(timestep))
        if tuple(sample.shape) != tuple(plan.sample.shape):
            raise ValueError(f"sample of shape {tuple(sample.shape)}, expected {tuple(plan.sample.shape)}")
        if encoder_hidden_states.dim() != 3 or encoder_hidden_states.shape[-1] != plan.enc.shape[1]:
            raise ValueError(f"encoder_hidden_states of shape {tuple(encoder_hidden_states.shape)}, expected "
                             f"[{plan.B}, {plan.L}, {plan.enc.shape[1]}]")
        s = sample.to(torch.float32)
        if cfg["center_input_sample"]:
            s = 2 * s - 1.0
        plan.sample.copy_(s, non_blocking=True)
        if in_scale is not None:
            plan.in_scale.fill_(float(in_scale))
        plan.enc.copy_(encoder_hidden_states.reshape(plan.B * plan.L, -1), non_blocking=True)
        if plan.image_embeds is not None:
            if added_cond_kwargs is None or "image_embeds" not in added_cond_kwargs:
                raise ValueError(f"{self.__class__} has the config param `encoder_hid_dim_type` set to 'ip_image_proj' which "
                                 "requires the keyword argument `image_embeds` to be passed in  `added_conditions`")
            ie = added_cond_kwargs["image_embeds"]
            if tuple(ie.shape) != tuple(plan.image_embeds.shape):
                raise ValueError(f"image_embeds of shape {tuple(ie.shape)}, expected {tuple(plan.image_embeds.shape)}")
            plan.image_embeds.copy_(ie, non_blocking=True)
        if cfg["addition_embed_type"] == "text_time":
            if added_cond_kwargs is None or "text_embeds" not in added_cond_kwargs:
                raise ValueError(f"{self.__class__} has the config param `addition_embed_type` set to 'text_time' which "
                                 "requires the keyword argument `text_embeds` to be passed in `added_cond_kwargs`")
            if "time_ids" not in added_cond_kwargs:
                raise ValueError(f"{self.__class__} has the config param `addition_embed_type` set to 'text_time' which "
                                 "requires the keyword argument `time_ids` to be passed in `added_cond_kwargs`")
            te, ti = added_cond_kwargs["text_embeds"], added_cond_kwargs["time_ids"]
            if plan.text_dim is None:
                self._finish_add_embedding(plan, te.shape[-1], ti.shape[-1])
            plan.add_in[:, :plan.text_dim].copy_(te, non_blocking=True)
            plan.time_ids.copy_(ti.reshape(-1).to(torch.float32), non_blocking=True)

    def forward(self, sample, timestep, encoder_hidden_states, class_labels=None, timestep_cond=None,
                attention_mask=None, cross_attention_kwargs=None, added_cond_kwargs=None,
                down_block_additional_residuals=None, mid_block_additional_residual=None,
                encoder_attention_mask=None, return_dict: bool = True, down_intrablock_additional_residuals=None):
        self_mask_len = 0
        if attention_mask is not None:
            if attention_mask.dim() != 2 or attention_mask.shape[0] != sample.shape[0]:
                raise ValueError(f"attention_mask: expected [batch, key_tokens], got {tuple(attention_mask.shape)}")
            self_mask_len = int(attention_mask.shape[1])
        # (class_labels without a class embedding are ignored, like unet_2d_condition.py:953)
        # T2I-Adapter residuals (unet_2d_condition.py:1078-1094): their own argument, or -- deprecated, kept like the reference keeps
        # it -- `down_block_additional_residuals` given without `mid_block_additional_residual`
        intra, deprecated = down_intrablock_additional_residuals, False
        if intra is None and down_block_additional_residuals is not None and mid_block_additional_residual is None:
            intra, down_block_additional_residuals, deprecated = down_block_additional_residuals, None, True
        controlnet = down_block_additional_residuals is not None
        if controlnet != (mid_block_additional_residual is not None):
            raise NotImplementedError("ControlNet residuals need both `down_block_additional_residuals` and "
                                      "`mid_block_additional_residual`")
        if intra is not None and controlnet:
            raise NotImplementedError("`down_intrablock_additional_residuals` (T2I-Adapter) together with ControlNet residuals in one "
                                      "forward is not implemented")
        intra = None if intra is None else list(intra)
        n_intra = 0 if intra is None else self._intrablock_count(intra, tuple(sample.shape), deprecated)
        ctrl = dict(down_block_additional_residuals=down_block_additional_residuals,
                    mid_block_additional_residual=mid_block_additional_residual, class_labels=class_labels,
                    timestep_cond=timestep_cond, attention_mask=attention_mask)
        if n_intra:
            ctrl["down_intrablock_additional_residuals"] = intra
        self.require_gpu(sample, encoder_hidden_states, *(intra or ()))
        B, _, H, W = sample.shape
        L = encoder_hidden_states.shape[1]
        if n_intra:
            plan = self._get_plan(B, H, W, L, encoder_attention_mask is not None, controlnet, self_mask_len, n_intra)
        else:
            plan = self._get_plan(B, H, W, L, encoder_attention_mask is not None, controlnet, self_mask_len)
        with self.on_stream():
            # in_scale = 1: forward() takes the sample as the model input. (A host that drives the same geometry through the staged API
            # with scale_model_input folded into conv_in -- bench.py does -- leaves its factor in the plan; round 5's bs-8 parity leg
            # read 0.68 instead of 1.2e-2 through exactly that.) The staged host's factor is put back afterwards: its
            # stage_inputs(in_scale=None) means "keep mine", not "whatever forward() left" (ADVICE r5).
            kept = plan.in_scale.clone()
            self.stage_inputs(plan, sample, timestep, encoder_hidden_states, added_cond_kwargs, in_scale=1.0,
                              encoder_attention_mask=encoder_attention_mask, **ctrl)
            out = self.run(plan).clone()
            plan.in_scale.copy_(kept)
        if not return_dict:
            return (out,)
        return UNet2DConditionOutput(sample=out)

    __call__ = forward


# ---------------------------------------------------------------------------------------------------------------- ControlNet
CONTROLNET_EXTRA_DEFAULTS = dict(conditioning_channels=3, conditioning_embedding_out_channels=(16, 32, 96, 256),
                                 controlnet_conditioning_channel_order="rgb", global_pool_conditions=False)


def _split_controlnet_config(config: Mapping):
    extra, base = dict(CONTROLNET_EXTRA_DEFAULTS), {}
    for k, v in config.items():
        if k.startswith("_"):
            continue
        (extra if k in CONTROLNET_EXTRA_DEFAULTS else base)[k] = v
    extra["conditioning_embedding_out_channels"] = tuple(extra["conditioning_embedding_out_channels"])
    if any(c % 8 for c in extra["conditioning_embedding_out_channels"]):
        raise ValueError("conditioning_embedding_out_channels must be multiples of 8")
    if extra["global_pool_conditions"]:
        raise NotImplementedError("ControlNetModel(mi355x): global_pool_conditions is not implemented")
    if extra["controlnet_conditioning_channel_order"] not in ("rgb", "bgr"):
        raise ValueError(f"unknown `controlnet_conditioning_channel_order`: {extra['controlnet_conditioning_channel_order']}")
    return base, extra


def controlnet_param_shapes(config: Mapping) -> Dict[str, tuple]:
    """name -> shape (Paddle layouts) of what ControlNetModel.forward reads (controlnet.py:262-417): the UNet's encoder half,
    the conditioning embedding (:81-101) and one 1x1 "zero convolution" per skip tensor plus one for the mid output."""
    base, extra = _split_controlnet_config(config)
    cfg = normalize_config(base)
    boc = cfg["block_out_channels"]
    S = {k: v for k, v in unet_param_shapes(base).items() if not k.startswith(("up_blocks.", "conv_norm_out.", "conv_out."))}

    def conv(name, i, o, k):
        S[name + ".weight"], S[name + ".bias"] = (o, i, k, k), (o,)

    ch = extra["conditioning_embedding_out_channels"]
    conv("controlnet_cond_embedding.conv_in", extra["conditioning_channels"], ch[0], 3)
    for i in range(len(ch) - 1):
        conv(f"controlnet_cond_embedding.blocks.{2 * i}", ch[i], ch[i], 3)
        conv(f"controlnet_cond_embedding.blocks.{2 * i + 1}", ch[i], ch[i + 1], 3)
    conv("controlnet_cond_embedding.conv_out", ch[-1], boc[0], 3)
    k = 0
    conv("controlnet_down_blocks.0", boc[0], boc[0], 1)
    for i, c in enumerate(boc):
        for _ in range(cfg["layers_per_block"][i] + (1 if i != len(boc) - 1 else 0)):
            k += 1
            conv(f"controlnet_down_blocks.{k}", c, c, 1)
    conv("controlnet_mid_block", boc[-1], boc[-1], 1)
    return S


def synth_controlnet_params(config: Mapping, seed: int = 1234, device="cpu") -> Dict[str, Tensor]:
    """random init like synth_unet_params (a trained ControlNet's zero convolutions are no longer zero either)"""
    g = torch.Generator(device=device).manual_seed(seed)
    P: Dict[str, Tensor] = {}
    for name, shape in controlnet_param_shapes(config).items():
        r = torch.randn(shape, generator=g, device=device)
        if name.endswith(".bias"):
            t = r * 0.02
        elif len(shape) == 1:
            t = 1.0 + r * 0.02
        elif len(shape) == 2:
            t = r / shape[0] ** 0.5
        else:
            t = r / (shape[1] * shape[2] * shape[3]) ** 0.5
        P[name] = t
    return P


class ControlNetOutput(SimpleNamespace):
    """``down_block_res_samples`` (tuple) and ``mid_block_res_sample`` (controlnet.py:46-68)"""


class _ControlNetWeights(_UNetWeights):
    def head(self):
        """in place of conv_norm_out / conv_out: the conditioning embedding and the zero convolutions"""
        ch = self.m._extra["conditioning_embedding_out_channels"]
        w = self.get("controlnet_cond_embedding.conv_in.weight")
        if self.m._extra["controlnet_conditioning_channel_order"] == "bgr":
            w = torch.flip(w, dims=[1])                               # flipping the input channels = flipping the weight's
        self.put_conv_in("cn.conv_in", w, "controlnet_cond_embedding.conv_in")
        for j in range(2 * (len(ch) - 1)):
            self.put_conv(f"cn.blocks.{j}", f"controlnet_cond_embedding.blocks.{j}")
        self.put_conv("cn.conv_out", "controlnet_cond_embedding.conv_out")
        k = 0
        while f"controlnet_down_blocks.{k}.weight" in self.shapes:
            self.put_conv(f"cn.down.{k}", f"controlnet_down_blocks.{k}")
            k += 1
        self.m._n_down = k
        self.put_conv("cn.mid", "controlnet_mid_block")


class _ControlNetPlanner(_UNetPlanner):
    def stem(self) -> _V:
        """ControlNetConditioningEmbedding.forward (controlnet.py:103-113) + ``sample = conv_in(sample) + cond`` (:807-810)"""
        x0 = super().stem()
        lib, stream, plan, pb, B, extra = self.lib, self.stream, self.plan, self.pb, self.B, self.m._extra
        ch = extra["conditioning_embedding_out_channels"]
        f = 1 << (len(ch) - 1)
        hc, wc = self.H * f, self.W * f
        plan.cond = pb.persist((B, extra["conditioning_channels"], hc, wc), torch.float32)
        bufs = [pb.persist((B * hc * wc * ch[0],), _lib.elem_dtype()), pb.persist((B * hc * wc * ch[0],), _lib.elem_dtype())]
        e = _V(bufs[0].data_ptr(), B * hc * wc, ch[0])
        pb.emit(lib.mi355x_sd_conv_in3x3, (plan.cond.data_ptr(), None, pb.wp("cn.conv_in.w"), pb.wp("cn.conv_in.b"), e.p, B,
                                           extra["conditioning_channels"], hc, wc, ch[0], e.ld, stream), "misc")
        pb.emit(lib.mi355x_sd_silu, (e.p, e.p, B * hc * wc * ch[0], 0, 0, stream), "misc")
        which = 0
        for i in range(len(ch) - 1):
            for j, (cout, stride) in enumerate(((ch[i], 1), (ch[i + 1], 2))):
                ho, wo = (hc + 2 - 3) // stride + 1, (wc + 2 - 3) // stride + 1
                which ^= 1
                out = _V(bufs[which].data_ptr(), B * ho * wo, cout)
                pb.conv3(e, hc, wc, f"cn.blocks.{2 * i + j}", out, stride=stride, flags=SILU)
                e, hc, wc = out, ho, wo
        assert (hc, wc) == (self.H, self.W)
        pb.conv3(e, hc, wc, "cn.conv_out", x0, R=x0)
        return x0

    def head(self, mid: _V, hm, wm):
        """zero convolutions + scaling (controlnet.py:842-869) -> fp32 NCHW residuals"""
        pb, B = self.pb, self.B
        scale, guess = self.m._cn_key
        n = len(self.skips)
        if n != self.m._n_down:
            raise ValueError(f"checkpoint has {self.m._n_down} controlnet_down_blocks, the configuration produces {n} skips")
        scales = [scale] * (n + 1)
        if guess:   # paddle.logspace(-1, 0, n + 1) * conditioning_scale (:855-859)
            scales = [float(v) * scale for v in torch.logspace(-1, 0, n + 1)]
        self.plan.ctrl_out = []
        for k, (cs, hs, ws_) in enumerate(self.skips + [(mid.C, hm, wm)]):
            sl = self.skip_slot(k) if k < n else mid
            rows = _V(pb.sc("cn_rows", 2 * sl.rows * cs), sl.rows, cs)
            pb.linear(sl, f"cn.down.{k}" if k < n else "cn.mid", rows, out_scale=scales[k])
            out = pb.persist((B, cs, hs, ws_), torch.float32)
            pb.emit(self.lib.mi355x_sd_unpatchify, (rows.p, rows.ld, B, cs, hs, ws_, 1, out.data_ptr(), self.stream), "misc")
            self.plan.ctrl_out.append(out)


class ControlNetModel(UNet2DConditionModel):
    """ControlNetModel.forward (PPD/models/controlnet.py:671-877) on the UNet's program: conv_in + conditioning embedding
    (3x3 convs with SiLU epilogues, the last one adding onto conv_in's output in place), the down blocks and the mid block
    exactly as in the UNet, then a 1x1 GEMM per skip tensor / mid output with ``conditioning_scale`` as its output scale,
    returned as the fp32 NCHW tensors ``UNet2DConditionModel.forward`` takes as ``down_block_additional_residuals`` /
    ``mid_block_additional_residual``."""
    _encoder_only = True
    _Weights, _Planner = _ControlNetWeights, _ControlNetPlanner
    _param_shapes = staticmethod(controlnet_param_shapes)

    def __init__(self, config: Mapping, params: Mapping[str, Tensor], **kw):
        base, self._extra = _split_controlnet_config(config)
        self._full_config = {k: v for k, v in config.items() if not k.startswith("_")}
        self._cn_key = (1.0, False)
        super().__init__(base, params, **kw)
        for k, v in self._extra.items():
            setattr(self.config, k, v)

    def _shapes(self) -> Dict[str, tuple]:
        return controlnet_param_shapes(self._full_config)

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float) -> None:
        raise ValueError("ControlNetModel has no up blocks: FreeU applies to the UNet2DConditionModel it conditions")

    def _get_plan(self, B, H, W, L, masked: bool = False, controlnet: bool = False) -> _Plan:
        return self.plan_for((B, H, W, L, masked) + self._cn_key, lambda: self._Planner(self, B, H, W, L, masked).build())

    def forward(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale: float = 1.0,
                class_labels=None, timestep_cond=None, attention_mask=None, added_cond_kwargs=None,
                cross_attention_kwargs=None, guess_mode: bool = False, return_dict: bool = True,
                encoder_attention_mask=None):
        if attention_mask is not None or cross_attention_kwargs:
            raise NotImplementedError("ControlNetModel(mi355x): attention_mask / cross_attention_kwargs are not implemented")
        if not isinstance(conditioning_scale, (int, float)):
            raise NotImplementedError("per-residual conditioning_scale lists are not implemented (a float is)")
        self.require_gpu(sample, encoder_hidden_states, controlnet_cond)
        B, _, H, W = sample.shape
        self._cn_key = (float(conditioning_scale), bool(guess_mode))
        plan = self._get_plan(B, H, W, encoder_hidden_states.shape[1], encoder_attention_mask is not None)
        if tuple(controlnet_cond.shape) != tuple(plan.cond.shape):
            raise ValueError(f"controlnet_cond of shape {tuple(controlnet_cond.shape)}, expected {tuple(plan.cond.shape)}")

        def stage(nb):
            self.stage_inputs(plan, sample, timestep, encoder_hidden_states, added_cond_kwargs, in_scale=1.0,
                              encoder_attention_mask=encoder_attention_mask, class_labels=class_labels,
                              timestep_cond=timestep_cond)
            plan.cond.copy_(controlnet_cond, non_blocking=nb)

        self.run_staged(plan, stage)
        outs = [t.clone() for t in plan.ctrl_out]
        if not return_dict:
            return tuple(outs[:-1]), outs[-1]
        return ControlNetOutput(down_block_res_samples=tuple(outs[:-1]), mid_block_res_sample=outs[-1])

    __call__ = forward
