"""CPU (-m "not gpu"): tiled AutoencoderKL decode / encode -- the tile split, the size classes batched through the untiled plan,
the pointer table and the one-pass blend -- executed by the host-memory ABI emulator against the restatement of the reference's
sequential tiled algorithm (tests/tiled_vae_ref.py), which is itself pinned once to the reference's own Python."""
import os

import numpy as np
import pytest
import torch

from oracle import vae_ref as R
from paddlemix_amd import vae as vae_mod
from paddlemix_amd.vae import AutoencoderKL, synth_decoder_params, synth_vae_params
from tests import tiled_vae_ref as TR
from tests.abi_emulator import on_emulator
from tests.abi_emulator_tiles import TileEmulator
from tests.configs import MINI_VAE

T, S = 16, 64
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_modules", "vae_tiled_mini.npz")


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def _bf(P):
    return {k: (v.to(torch.bfloat16).float() if v.dim() > 1 else v) for k, v in P.items()}


def _z(*shape, seed=1):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def P():
    return synth_vae_params(MINI_VAE, seed=7)


def _model(P, cfg=MINI_VAE, f=None):
    vae = on_emulator(AutoencoderKL, cfg, P, backend=TileEmulator())
    vae.tile_latent_min_size, vae.tile_sample_min_size = T, S
    if f is not None:
        vae.tile_overlap_factor = f
    vae.enable_tiling()
    return vae


def test_restatement_reproduces_the_reference_python():
    """tests/golden/reference_modules/vae_tiled_mini.npz is the reference's AutoencoderKL.tiled_decode / tiled_encode itself
    (scripts/record_vae_tiling_golden.py): z [1,4,32,25] -> tile widths 16, 13, 1"""
    from tests import reference_cases as RC
    gold = np.load(GOLD)
    dec_seed, enc_seed = (int(v) for v in gold["seeds"])
    t, s = (int(v) for v in gold["tile"])
    Pg = R.synth_decoder_params(MINI_VAE, seed=dec_seed)
    Pg.update(RC._synth(R.encoder_param_shapes(MINI_VAE), enc_seed))
    with torch.no_grad():
        dec = TR.tiled_decode(Pg, MINI_VAE, torch.from_numpy(gold["z"]), t, s)
        mean, logvar, _ = TR.tiled_encode(Pg, MINI_VAE, torch.from_numpy(gold["img"]), t, s)
    for got, key in ((dec, "decode"), (mean, "encode_mean"), (logvar, "encode_logvar")):
        g = torch.from_numpy(gold[key])
        assert got.shape == g.shape and _rel(got, g) < 4.7e-6, (key, _rel(got, g))


@pytest.mark.parametrize("H,W,S_,lim,ext", [(100, 128, 64, 48, 16),     # row extents 64, 52, 4: the second-to-last tile is short as well
                                            (128, 100, 64, 48, 16),     # the same on the column axis
                                            (96, 160, 64, 32, 32),      # f = 0.5: the bands fill the kept part of a tile
                                            (50, 39, 24, 18, 6)])       # nothing a multiple of 4
def test_closed_form_is_the_sequential_algorithm(H, W, S_, lim, ext):
    """what the kernel is specified as (the emulator's fp32 closed form) and what its GPU test measures against (the float64 closed
    form) are both the reference's sequential in-place blend, corners included: bit for bit, not to a tolerance"""
    g = torch.Generator().manual_seed(H + W)
    ny, nx = -(-H // lim), -(-W // lim)
    rows = [[torch.randn(2, 3, min(S_, H - i * lim), min(S_, W - j * lim), generator=g) for j in range(nx)] for i in range(ny)]
    seq = TR.blend_tiles(rows, ext, lim)
    assert seq.shape == (2, 3, H, W)
    val, mag, band = TR.blend_closed_form64(rows, H, W, S_, lim, ext)
    assert torch.equal(val, TR.blend_tiles([[t.double() for t in r] for r in rows], ext, lim))
    assert band.any() and (~band).any() and (mag >= val.abs()).all()
    assert ((seq.double() - val).abs() <= 16 * 2.0 ** -24 * mag).all()          # the GPU test's bound holds for the reference itself
    table = torch.tensor([[t.data_ptr() + 4 * b * t.stride(0) for r in rows for t in r] for b in range(2)], dtype=torch.int64)
    out = torch.empty(2, 3, H, W)
    assert TileEmulator().mi355x_sd_tile_blend(table.data_ptr(), 2, 3, H, W, S_, lim, ext, ny, nx, 1, 0, 1, out.data_ptr(),
                                               3 * H * W, H * W, W, 1, 0) == 0
    assert torch.equal(out, seq)


def test_defaults_and_switches(P):
    vae = on_emulator(AutoencoderKL, MINI_VAE, P, backend=TileEmulator())
    assert vae.use_tiling is False and vae.tile_overlap_factor == 0.25
    assert vae.tile_sample_min_size == 512 and vae.tile_latent_min_size == 128     # sample_size / 2^(levels - 1), three levels
    vae.enable_tiling()
    assert vae.use_tiling is True
    vae.enable_tiling(False)
    assert vae.use_tiling is False
    vae.enable_tiling()
    vae.disable_tiling()
    assert vae.use_tiling is False


@pytest.mark.parametrize("shape,f", [((2, 4, 32, 28), 0.25),      # tiles 16 / 16 / 8 x 16 / 16 / 4
                                     ((2, 4, 32, 25), 0.25),      # widths 16, 13, 1: the second-to-last tile is short as well
                                     ((1, 4, 24, 40), 0.5)])
def test_tiled_decode_matches_the_restatement(P, shape, f):
    vae, z = _model(P, f=f), _z(*shape)
    out = vae.decode(z).sample
    ref = TR.tiled_decode(_bf(P), MINI_VAE, z, T, S, f)
    assert out.shape == ref.shape == (shape[0], 3, 4 * shape[2], 4 * shape[3]) and out.dtype == torch.float32
    assert _rel(out, ref) <= 2e-2, _rel(out, ref)
    assert "tile_blend" in vae._lib.calls and "tile_gather" in vae._lib.calls
    if shape == (2, 4, 32, 28):
        # the bar separates the tiled result from its neighbours by more than 10x: untiled, and tiled without the blend
        vae.disable_tiling()
        assert _rel(vae.decode(z).sample, ref) > 0.1
        assert _rel(TR.tiled_decode(_bf(P), MINI_VAE, z, T, S, f, blend=False), ref) > 0.1


def test_tiled_decode_in_scale_tuple_slicing_and_repeat(P):
    vae, z = _model(P), _z(2, 4, 32, 28, seed=3)
    ref = TR.tiled_decode(_bf(P), MINI_VAE, z, T, S, scaled=True)
    out = vae.decode(z, return_dict=False, in_scale=1.0 / MINI_VAE["scaling_factor"])
    assert isinstance(out, tuple) and _rel(out[0], ref) <= 2e-2
    n_plans, n_tilings = len(vae._plans), len(vae._tilings)
    again = vae.decode(z, return_dict=False, in_scale=1.0 / MINI_VAE["scaling_factor"])[0]
    assert torch.equal(again, out[0]) and again.data_ptr() != out[0].data_ptr()
    assert (len(vae._plans), len(vae._tilings)) == (n_plans, n_tilings)       # same geometry: nothing is planned again
    assert torch.equal(vae.tiled_decode(z, in_scale=1.0 / MINI_VAE["scaling_factor"]).sample, again)
    # every size class ran as ONE batch over both images: 2 * (4, 2, 2, 1) tiles
    assert sorted(k[1] for k in vae._plans if k[0] == "decode") == [2, 4, 4, 8]
    vae.enable_slicing()                                                        # the cut is one image's tiles
    sl = vae.decode(z, in_scale=1.0 / MINI_VAE["scaling_factor"]).sample
    assert _rel(sl, ref) <= 2e-2 and _rel(sl, again) <= 2e-2
    assert sorted(k[1] for k in vae._plans if k[0] == "decode") == [1, 2, 2, 2, 4, 4, 4, 8]


def test_batch_cut_by_the_activation_limit_collects_the_slices(P, monkeypatch):
    vae, z = _model(P), _z(2, 4, 32, 28, seed=4)
    whole = vae.decode(z).sample
    monkeypatch.setattr(vae_mod, "_MAX_ELEMS", 3 * 64 * 64 * 64)               # three full tiles per launch sequence
    cut = _model(P)
    out = cut.decode(z).sample
    assert any(c.stack is not None for t in cut._tilings.values() for c in t.classes)
    assert _rel(out, whole) <= 2e-2 and _rel(out, TR.tiled_decode(_bf(P), MINI_VAE, z, T, S)) <= 2e-2


def test_input_within_one_tile_takes_the_untiled_path(P):
    vae, z = _model(P), _z(2, 4, 16, 12)
    on = vae.decode(z).sample
    assert "tile_blend" not in vae._lib.calls
    vae.disable_tiling()
    assert torch.equal(vae.decode(z).sample, on)
    x = torch.rand(1, 3, 64, 48, generator=torch.Generator().manual_seed(5)) * 2 - 1
    off = vae.encode(x).latent_dist.mean
    vae.enable_tiling()
    assert torch.equal(vae.encode(x).latent_dist.mean, off) and "tile_blend" not in vae._lib.calls


def test_tiled_encode_matches_the_restatement(P):
    vae = _model(P)
    g = torch.Generator().manual_seed(6)
    x = torch.rand(2, 3, 128, 112, generator=g) * 2 - 1
    post = vae.encode(x).latent_dist
    assert post.mean.shape == (2, 4, 32, 28)
    noise = torch.randn(post.mean.shape, generator=g)
    mean, logvar, sample = TR.tiled_encode(_bf(P), MINI_VAE, x, T, S, noise=noise)
    assert _rel(post.mean, mean) <= 2e-2 and _rel(post.logvar, logvar) <= 2e-2
    got = post.sample(noise=noise)
    assert _rel(got, sample) <= 2e-2
    assert torch.allclose(got, post.mean + post.std * noise, atol=1e-5)
    assert vae.encode(x, return_dict=False)[0].mean.equal(post.mean)
    assert vae.tiled_encode(x).latent_dist.logvar.equal(post.logvar)
    assert _rel(post.mean, R.encode(_bf(P), MINI_VAE, x)[0]) > 0.1             # not the untiled posterior


def test_refusals_name_the_value(P):
    z = _z(1, 4, 32, 28)
    for f in (-0.1, 0.6):
        with pytest.raises(ValueError, match="tile_overlap_factor = " + str(f)):
            _model(P, f=f).decode(z)
    vae = _model(P)
    vae.tile_latent_min_size, vae.tile_sample_min_size = 1, 4                  # stride int(1 * 0.75) = 0
    with pytest.raises(ValueError, match="= 0 must be at least 1"):
        vae.decode(z)
    vae.tile_latent_min_size, vae.tile_sample_min_size = 16, 60                # 12 * 4 = 48 latent-stride pixels, 45 kept
    with pytest.raises(ValueError, match="tile_sample_min_size = 60"):
        vae.decode(z)
    with pytest.raises(ValueError, match="tile_sample_min_size = 60"):
        vae.encode(torch.zeros(1, 3, 128, 112))
    vae.tile_latent_min_size, vae.tile_sample_min_size = 8, 32                 # 20 x 14 -> heights 8, 8, 8, 2 and widths 8, 8, 2
    with pytest.raises(ValueError, match=r"tile \(3, 2\) has a 2 x 2 latent"):
        vae.decode(_z(1, 4, 20, 14))
    vae.tile_latent_min_size, vae.tile_sample_min_size = T, S
    with pytest.raises(ValueError, match=r"tile \(0, 2\) of the image is 64 x 18"):
        vae.encode(torch.zeros(1, 3, 64, 114))
    assert "tile_gather" not in vae._lib.calls                                 # all of it before any launch
    with pytest.raises(ValueError):
        vae.tiled_decode(torch.zeros(1, 3, 32, 28))


def test_models_that_cannot_tile():
    cfg = dict(MINI_VAE, use_post_quant_conv=False)
    vae = on_emulator(AutoencoderKL, cfg, synth_decoder_params(cfg, seed=3), backend=TileEmulator())
    with pytest.raises(NotImplementedError):
        vae.enable_tiling()
    with pytest.raises(NotImplementedError):
        vae.tiled_decode(_z(1, 4, 32, 28))
    from paddlemix_amd._lib import MI355XError
    dec_only = on_emulator(AutoencoderKL, MINI_VAE, synth_decoder_params(MINI_VAE, seed=3), backend=TileEmulator())
    with pytest.raises(MI355XError):
        dec_only.tiled_encode(torch.zeros(1, 3, 128, 112))
    cfg = dict(MINI_VAE, use_quant_conv=False)
    no_q = on_emulator(AutoencoderKL, cfg, synth_vae_params(cfg, seed=3), backend=TileEmulator())
    with pytest.raises(NotImplementedError):
        no_q.tiled_encode(torch.zeros(1, 3, 128, 112))


def test_pipeline_switches_reach_the_model(P):
    from paddlemix_amd.pipeline import DiTDenoiser, StableDiffusion3Denoiser, StableDiffusionDenoiser
    for make in (lambda v: StableDiffusionDenoiser(None, None, vae=v), lambda v: StableDiffusion3Denoiser(None, None, vae=v),
                 lambda v: DiTDenoiser(None, None, vae=v)):
        vae = on_emulator(AutoencoderKL, MINI_VAE, P, backend=TileEmulator())
        pipe = make(vae)
        pipe.enable_vae_tiling()
        pipe.enable_vae_slicing()
        assert vae.use_tiling and vae.use_slicing
        pipe.disable_vae_tiling()
        pipe.disable_vae_slicing()
        assert not vae.use_tiling and not vae.use_slicing
        with pytest.raises(ValueError):
            make(None).enable_vae_tiling()
