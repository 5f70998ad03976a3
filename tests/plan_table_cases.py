"""The planner outputs that tests/test_plan_tables.py holds to tests/golden/plan_tables.json: every model family and planner
mode, built and run once on the host-memory emulator.

    record(name) -> [ {launches, prog: [[symbol, kind, flops], ...], tables_sha256}, ... ]     one entry per cached plan, in the
                                                                                              order the model planned them

`tables_sha256` is over the exported program's tables (paddlemix_amd/export.py: region table, I/O table and launch list with every
pointer rewritten as (region, byte offset)) without the fixed 40-byte header, so it pins argument values, scratch sharing and
buffer order, and an ABI bump does not move it.

    python -m tests.plan_table_cases tests/golden/plan_tables.json COMMIT      writes the fixture: done once, on the commit before
                                                                               the planners moved onto PlanBuilder, which it names
A case of a model that came later is recorded on its own into tests/golden/plan_tables_later.json (same layout, `recorded_at` the
commit it was taken on), so that the first fixture stays as recorded."""
import hashlib
import json
import os
import struct
import sys
import tempfile

import torch

from tests import configs as C
from tests import export_cases as EC
from tests.abi_emulator import on_emulator

_HEADER = 8 + struct.calcsize("<IIIIIIQ")


def _unet(cfg, x_hw=(16, 16), ctor_kw=None, **fkw):
    def build():
        from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
        g = torch.Generator().manual_seed(7)
        m = UNet2DConditionModel(cfg, synth_unet_params(cfg, seed=1), **(ctor_kw or {}))
        x, enc = torch.randn(2, 4, *x_hw, generator=g), torch.randn(2, 7, cfg["cross_attention_dim"], generator=g)
        kw = {k: (v(g) if callable(v) else v) for k, v in fkw.items()}
        return m, (lambda: m(x, 501, enc, **kw)), ("out",)
    return build


def _exported(name, after_build=None, **kw):
    def build():
        m, run, outputs = EC.build(name, True, **kw)
        if after_build:
            after_build(m)
        return m, run, outputs
    return build


def _controlnet_guess():
    from paddlemix_amd.unet import ControlNetModel, synth_controlnet_params
    g = torch.Generator().manual_seed(7)
    m = ControlNetModel(C.TINY, synth_controlnet_params(C.TINY, seed=3))
    x, enc, cond = torch.randn(1, 4, 16, 16, generator=g), torch.randn(1, 7, 64, generator=g), torch.randn(1, 3, 128, 128, generator=g)
    return m, (lambda: m(x, 20, enc, cond, conditioning_scale=0.7, guess_mode=True)), ("ctrl_out",)


def _vae_tiled():
    """one tiled decode whose 32 x 28 latent splits into tiles of 16 / 16 / 8 x 16 / 16 / 4: four size classes, four plans"""
    from paddlemix_amd.vae import AutoencoderKL, synth_vae_params
    m = AutoencoderKL(C.MINI_VAE, synth_vae_params(C.MINI_VAE, 9))
    m.tile_latent_min_size, m.tile_sample_min_size, m.tile_overlap_factor = 16, 64, 0.25
    m.enable_tiling()
    z = torch.randn(2, 4, 32, 28, generator=torch.Generator().manual_seed(7))
    return m, (lambda: m.decode(z)), ("out",)


def _vae_no_post_quant():
    from paddlemix_amd.vae import AutoencoderKL, synth_vae_params
    cfg = dict(C.MINI_VAE, use_post_quant_conv=False)
    m = AutoencoderKL(cfg, synth_vae_params(cfg, 9))
    z = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(7))
    return m, (lambda: m.decode(z, in_scale=1.0 / cfg["scaling_factor"])), ("out",)


_rn = lambda *s: (lambda g: torch.randn(*s, generator=g))  # noqa: E731
_TED = 4 * C.TINY["block_out_channels"][0]

CASES = {name: _exported(name) for name in EC.NAMES}
CASES.update({
    "unet_tiny+resid_fp32": _exported("unet_tiny", residual_dtype="fp32"),
    "unet_tiny+fold_layernorm": _exported("unet_tiny", fold_layernorm=True),
    "unet_tiny+no_fold_softmax_scale": _exported("unet_tiny", fold_softmax_scale=False),
    "unet_ip_adapter+scale0": _exported("unet_ip_adapter", after_build=lambda m: m.set_ip_adapter_scale(0.0)),
    "sd3_mini+fp8w": _exported("sd3_mini", weight_dtype="fp8"),
    "sd3_mini+w8a8": _exported("sd3_mini", weight_dtype="fp8", act_dtype="fp8"),
    "vae_tiled_decode": _vae_tiled,
    # planner branches that none of the cases above reaches
    "unet_mini_xl+no_fold_softmax_scale": _exported("unet_mini_xl", fold_softmax_scale=False),   # head_dim 64: the non-log2 attention
    "unet_mini_xl+resid_fp32": _exported("unet_mini_xl", residual_dtype="fp32"),
    "unet_tiny+self_mask": _unet(C.TINY, attention_mask=torch.ones(2, 64)),
    "unet_tiny_hd64+self_mask": _unet(dict(C.TINY, attention_head_dim=2), attention_mask=torch.ones(2, 64)),   # log2 scores + a bias
    "unet_tiny+odd_latent": _unet(C.TINY, x_hw=(15, 13)),                                     # cropped nearest upsampling
    "unet_tiny+class_embedding_concat": _unet(dict(C.TINY, num_class_embeds=10, class_embeddings_concat=True),
                                              class_labels=torch.tensor([3, 8])),
    "unet_tiny+class_timestep_concat": _unet(dict(C.TINY, class_embed_type="timestep", class_embeddings_concat=True),
                                             class_labels=torch.tensor([3.0, 8.0])),
    "unet_tiny+class_projection": _unet(dict(C.TINY, class_embed_type="projection", projection_class_embeddings_input_dim=32),
                                        class_labels=_rn(2, 32)),
    "unet_tiny+class_simple_projection+tcond": _unet(dict(C.TINY, class_embed_type="simple_projection",
                                                          projection_class_embeddings_input_dim=32, time_cond_proj_dim=32),
                                                     class_labels=_rn(2, 32), timestep_cond=_rn(2, 32)),
    "unet_tiny+class_identity": _unet(dict(C.TINY, class_embed_type="identity"), class_labels=_rn(2, _TED)),
    "unet_tiny+class_identity_concat": _unet(dict(C.TINY, class_embed_type="identity", class_embeddings_concat=True),
                                             class_labels=_rn(2, _TED)),
    "controlnet_tiny+guess_mode": _controlnet_guess,
    "vae_decode+no_post_quant_conv": _vae_no_post_quant,
})


def tables_digest(path: str) -> str:
    """sha256 of an exported program's tables: the file from the end of its fixed header up to the first region's contents"""
    raw = open(path, "rb").read()
    n_regions = struct.unpack_from("<I", raw, 8 + 12)[0]
    pos, first = _HEADER, len(raw)
    for _ in range(n_regions):
        _, _, off = struct.unpack_from("<IQQ", raw, pos)
        pos += 20
        pos += 4 + struct.unpack_from("<I", raw, pos)[0]
        if off:
            first = min(first, off)
    return hashlib.sha256(raw[_HEADER:first]).hexdigest()


def record(name: str) -> list:
    from paddlemix_amd.export import export_program
    backend = None
    if name == "vae_tiled_decode":   # the emulator that also has the tile gather / blend entry points
        from tests.abi_emulator_tiles import TileEmulator
        backend = TileEmulator()
    model, run, outputs = on_emulator(CASES[name], backend=backend)
    run()
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, plan in enumerate(model._plans.values()):
            path = os.path.join(tmp, f"{i}.mi3prg")
            export_program(model, plan, path, outputs)
            out.append(dict(launches=len(plan.prog), prog=[[fn.__name__, kind, flops] for fn, _, kind, flops in plan.prog],
                            tables_sha256=tables_digest(path)))
    return out


if __name__ == "__main__":
    torch.manual_seed(0)
    with open(sys.argv[1], "w") as fh:
        json.dump(dict(recorded_at=sys.argv[2], cases={name: record(name) for name in CASES}), fh, separators=(",", ":"))
        fh.write("\n")
