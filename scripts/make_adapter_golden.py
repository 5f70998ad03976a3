"""Record tests/golden/adapter/*.npz from the reference's own code (build container only: needs the reference checkout).

    python scripts/make_adapter_golden.py

Runs the reference's unmodified ``models/adapter.py`` (T2IAdapter, MultiAdapter) and ``UNet2DConditionModel.forward`` with
``down_intrablock_additional_residuals`` over oracle/paddle_shim.py on the cases of tests/adapter_cases.py and stores their outputs.
The shim has no ``nn.PixelUnshuffle``: this script attaches one to the shim's ``nn`` (torch's pixel_unshuffle, the same index map) before
the reference module is imported. The shim's ``AvgPool2D`` ignores ``ceil_mode``, so ONLY geometries whose pooled sizes are all even are
recorded -- there ceil mode changes nothing; odd geometries are pinned by the torch restatement alone (tests/adapter_ref.py)."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import paddle_shim, reference_runner as RR   # noqa: E402
from tests import adapter_cases as AC   # noqa: E402
from tests import adapter_ref as AR   # noqa: E402


class PixelUnshuffle(paddle_shim.Layer):
    def __init__(self, downscale_factor, data_format="NCHW", name=None):
        super().__init__()
        assert data_format == "NCHW"
        self.downscale_factor = downscale_factor

    def forward(self, x):
        return paddle_shim.Tensor(TF.pixel_unshuffle(x.t, self.downscale_factor))


def reference_adapter(config, params):
    shim = RR.install()
    shim["paddle.nn"].PixelUnshuffle = PixelUnshuffle
    m = RR.ref_module("adapter")
    net = m.T2IAdapter(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in config.items()})
    return RR.load_params(net, params), m


def even_all_the_way(config, H, W):
    cfg = AR.normalize_adapter_config(config)
    h, w = H // cfg["downscale_factor"], W // cfg["downscale_factor"]
    for _, _, down in AR._blocks(cfg):
        if down:
            if h % 2 or w % 2:
                return False
            h, w = h // 2, w // 2
    return True


def main():
    os.makedirs(AC.GOLDEN, exist_ok=True)
    index = {}
    nets = {}
    for name, (B, H, W) in AC.ADAPTER_GOLDEN.items():
        config = AR.ADAPTERS[name]
        assert even_all_the_way(config, H, W), (name, H, W)
        P = AR.synth_adapter_params(config, seed=21)
        net, mod = reference_adapter(config, P)
        nets[name] = net
        x = AC.image(B, config["in_channels"], H, W)
        feats = RR.from_shim(net(RR.to_shim(x)))
        out = {f"feature_{i}": f.numpy() for i, f in enumerate(feats)}
        out["total_downscale_factor"] = np.array(net.total_downscale_factor)
        out["downscale_factor"] = np.array(net.downscale_factor)
        np.savez(os.path.join(AC.GOLDEN, f"adapter_{name}.npz"), **out)
        index[f"adapter_{name}"] = dict(config={k: (list(v) if isinstance(v, tuple) else v) for k, v in config.items()}, image=[B, H, W])
    # MultiAdapter: two full adapters (seeds 21, 22), weights (0.7, 0.4)
    config = AR.ADAPTERS["full"]
    B, H, W = AC.ADAPTER_GOLDEN["full"]
    second, mod = reference_adapter(config, AR.synth_adapter_params(config, seed=22))
    multi = mod.MultiAdapter([nets["full"], second])
    xs = [AC.image(B, 3, H, W, seed=11), AC.image(B, 3, H, W, seed=12)]
    feats = RR.from_shim(multi(RR.to_shim(xs), [0.7, 0.4]))
    np.savez(os.path.join(AC.GOLDEN, "multi_adapter_full.npz"), **{f"feature_{i}": f.numpy() for i, f in enumerate(feats)})
    index["multi_adapter_full"] = dict(seeds=[21, 22], adapter_weights=[0.7, 0.4], image_seeds=[11, 12])
    # the U-Net with intrablock residuals: the forms of tests/adapter_cases.unet_golden_forms, the deprecated argument, none
    for name in AC.UNET_GOLDEN:
        cfg, P, (sample, enc, added), res = AC.unet_golden_inputs(name)
        net = RR.build_unet(cfg, P)
        call = lambda **kw: RR.from_shim(net(RR.to_shim(sample), AC.T, RR.to_shim(enc), added_cond_kwargs=RR.to_shim(added),  # noqa: E731
                                             return_dict=False, **kw)[0]).numpy()
        clone = lambda rs: RR.to_shim([r.clone() for r in rs])  # noqa: E731
        forms = AC.unet_golden_forms(res, len(cfg["block_out_channels"]))
        out = {k: call(down_intrablock_additional_residuals=clone(v)) for k, v in forms.items()}
        out["plain"] = call()
        out["deprecated"] = call(down_block_additional_residuals=clone(forms["intrablock"]))
        np.savez(os.path.join(AC.GOLDEN, f"unet_{name}.npz"), **out)
        index[f"unet_{name}"] = dict(latents=list(AC.UNET_GOLDEN[name]), timestep=AC.T, residual_seed=7, residual_scale=0.5)
    with open(os.path.join(AC.GOLDEN, "index.json"), "w") as fh:
        json.dump(index, fh, indent=1, sort_keys=True)
    print("wrote", sorted(os.listdir(AC.GOLDEN)))


if __name__ == "__main__":
    main()
