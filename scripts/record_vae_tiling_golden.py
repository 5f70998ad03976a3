"""Record tests/golden/reference_modules/vae_tiled_mini.npz: the reference's own AutoencoderKL.tiled_decode / tiled_encode
(ppdiffusers/models/autoencoder_kl.py) run through the Paddle shim (oracle/reference_runner.py) on the mini VAE with small tiles.
Needs the reference checkout (reference_runner.available()); the test that reads the file (tests/test_vae_tiling_host_logic.py)
does not. Parameters are not stored: they are oracle.vae_ref's synthetic ones for the recorded seeds.

    python scripts/record_vae_tiling_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import reference_runner as rr  # noqa: E402
from oracle import vae_ref as V  # noqa: E402
from tests import reference_cases as RC  # noqa: E402
from tests.configs import MINI_VAE  # noqa: E402

DEC_SEED, ENC_SEED, T, S = 2, 7, 16, 64


def params():
    P = V.synth_decoder_params(MINI_VAE, seed=DEC_SEED)
    P.update(RC._synth(V.encoder_param_shapes(MINI_VAE), ENC_SEED))
    return P


def main():
    if not rr.available():
        raise SystemExit("the reference checkout is not available here")
    P = params()
    g = torch.Generator().manual_seed(11)
    z, img = torch.randn(1, 4, 32, 25, generator=g), torch.randn(1, 3, 128, 100, generator=g)
    full = V.normalize_config(MINI_VAE)
    n = len(full["block_out_channels"])
    full.update(down_block_types=("DownEncoderBlock2D",) * n, up_block_types=("UpDecoderBlock2D",) * n)
    full.pop("use_post_quant_conv", None)
    full.pop("use_quant_conv", None)
    with torch.no_grad():
        net = rr.ref_module("autoencoder_kl").AutoencoderKL(**full)
        net.eval()
        rr.load_params(net, P)
        net.tile_latent_min_size, net.tile_sample_min_size = T, S
        net.enable_tiling()
        dec = rr.from_shim(net.decode(rr.to_shim(z)).sample)
        post = net.encode(rr.to_shim(img)).latent_dist
        mean, logvar = rr.from_shim(post.mean), rr.from_shim(post.logvar)
    path = os.path.join(ROOT, "tests", "golden", "reference_modules", "vae_tiled_mini.npz")
    np.savez_compressed(path, z=z.numpy(), img=img.numpy(), decode=dec.numpy(), encode_mean=mean.numpy(), encode_logvar=logvar.numpy(),
                        seeds=np.array([DEC_SEED, ENC_SEED]), tile=np.array([T, S]))
    print(path, os.path.getsize(path), tuple(dec.shape), tuple(mean.shape))


if __name__ == "__main__":
    main()
