"""GPU: the two tiled-VAE kernels (csrc/tiles.hip) element by element, and tiled AutoencoderKL decode / encode against the
restatement of the reference's sequential tiled algorithm (tests/tiled_vae_ref.py)."""
import pytest
import torch

from tests import tiled_vae_ref as TR
from tests.configs import MINI_VAE, SD_VAE

pytestmark = pytest.mark.gpu

# a 3 x 3 grid with row extents (64, 52, 4) and column extents (64, 64, 32): the second-to-last row tile is short as well
B, C, H, W, S, LIM, EXT = 2, 3, 100, 128, 64, 48, 16


@pytest.fixture(scope="module")
def ops():
    from paddlemix_amd import ops as o
    o.init(0)
    return o


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _tiles(kind, c=C):
    g = torch.Generator().manual_seed(5)
    rows = []
    for i in range(3):
        rows.append([])
        for j in range(3):
            shape = (B, c, min(S, H - i * LIM), min(S, W - j * LIM))
            rows[-1].append(torch.randn(shape, generator=g) if kind == "normal" else torch.full(shape, float(1 + 3 * i + j)) +
                            torch.arange(B * c, dtype=torch.float32).reshape(B, c, 1, 1) * 16)
    return rows


def _check_blend(out, rows):
    """bit-equal to the source tile outside the bands; inside, |out - ref64| <= 16 * 2^-24 * sum_k w_k |D_k|: three nested fp32
    lerps, each with at most 2 weight roundings, 2 products and 1 sum (contracted or not) -> at most 5 roundings of relative size
    2^-24 per level on a quantity bounded by sum_k w_k |D_k|, 15 in all, rounded up to 16"""
    ref, mag, band = TR.blend_closed_form64(rows, H, W, S, LIM, EXT)
    out = out.double()
    assert band.sum().item() == 5120 and (~band).any()
    assert torch.equal(out[:, :, ~band], ref[:, :, ~band])
    err, bound = (out - ref).abs()[:, :, band], (16 * 2.0 ** -24 * mag)[:, :, band]
    print(f"tile_blend: max err / bound in the bands = {(err / bound.clamp_min(1e-30)).max().item():.3f}")
    assert (err <= bound).all()
    seq = TR.blend_tiles(rows, EXT, LIM)   # the reference's sequential in-place fp32 algorithm itself: same products, same sums
    differ = (out.float() != seq).sum().item()
    print(f"tile_blend: elements that differ from the sequential fp32 algorithm: {differ}")
    assert differ == 0


@pytest.mark.parametrize("kind", ["normal", "constant"])
def test_tile_blend_nchw(ops, kind):
    rows = _tiles(kind)
    out = ops.tile_blend([[t.cuda() for t in r] for r in rows], H, W, S, LIM, EXT).cpu()
    assert out.shape == (B, C, H, W)
    _check_blend(out, rows)


def test_tile_blend_unaligned_rows_take_the_scalar_path(ops):
    """extents that are no multiple of 4 (W = 126: the last column tile is 30 wide)"""
    g = torch.Generator().manual_seed(6)
    w = 126
    rows = [[torch.randn(1, 2, min(S, H - i * LIM), min(S, w - j * LIM), generator=g) for j in range(3)] for i in range(3)]
    out = ops.tile_blend([[t.cuda() for t in r] for r in rows], H, w, S, LIM, EXT).cpu().double()
    ref, mag, band = TR.blend_closed_form64(rows, H, w, S, LIM, EXT)
    assert torch.equal(out[:, :, ~band], ref[:, :, ~band])
    assert ((out - ref).abs() <= 16 * 2.0 ** -24 * mag).all()


@pytest.mark.parametrize("kind", ["normal", "constant"])
def test_tile_blend_token_major(ops, kind):
    """the encoder's layout: every tile fp32 rows [B, eh * ew, 8], the result rows [B, H * W, 8]"""
    rows = _tiles(kind, c=8)
    tok = [[t.permute(0, 2, 3, 1).reshape(B, -1, 8).contiguous().cuda() for t in r] for r in rows]
    out = ops.tile_blend(tok, H, W, S, LIM, EXT, token_major=True).cpu()
    assert out.shape == (B, H * W, 8)
    out = out.reshape(B, H, W, 8).permute(0, 3, 1, 2)
    ref, mag, band = TR.blend_closed_form64(rows, H, W, S, LIM, EXT)
    assert torch.equal(out.double()[:, :, ~band], ref[:, :, ~band])
    assert ((out.double() - ref).abs() <= 16 * 2.0 ** -24 * mag).all()


def test_tile_gather_is_slicing(ops):
    g = torch.Generator().manual_seed(7)
    for (h, w, y0, x0, st, ny, nx, wh, ww) in ((32, 28, 0, 0, 12, 2, 2, 16, 16),     # 16-byte rows
                                               (32, 25, 0, 12, 12, 2, 1, 16, 13),    # odd widths: scalar path
                                               (32, 25, 24, 24, 12, 1, 1, 8, 1),     # the 1-column tile
                                               (320, 272, 0, 0, 96, 3, 2, 128, 128)):
        x = torch.randn(2, 3, h, w, generator=g)
        ref = torch.stack([x[b, :, y0 + iy * st:y0 + iy * st + wh, x0 + ix * st:x0 + ix * st + ww]
                           for b in range(2) for iy in range(ny) for ix in range(nx)])
        out = ops.tile_gather(x.cuda(), (y0, x0), (st, st), (ny, nx), (wh, ww))
        assert torch.equal(out.cpu(), ref)
        n = ref.shape[0]
        if n > 2:   # a slice of the stack
            assert torch.equal(ops.tile_gather(x.cuda(), (y0, x0), (st, st), (ny, nx), (wh, ww), first=1, count=n - 2).cpu(), ref[1:n - 1])


def test_argument_errors(ops):
    from paddlemix_amd._lib import MI355XError
    rows = [[t.cuda() for t in r] for r in _tiles("constant")]
    with pytest.raises(MI355XError, match="ext <= lim"):
        ops.tile_blend(rows, H, W, S, LIM, LIM + 4)                            # a blend would read the neighbour's own band
    x = torch.zeros(1, 3, 32, 28, device="cuda")
    with pytest.raises(MI355XError, match="leaves the source"):
        ops.tile_gather(x, (0, 0), (12, 12), (3, 2), (16, 16))                 # 24 + 16 > 32
    with pytest.raises(MI355XError, match="positive"):
        ops.tile_gather(x, (0, 0), (12, 12), (0, 2), (16, 16), count=1)
    with pytest.raises(MI355XError, match="range"):
        ops.tile_gather(x, (0, 0), (12, 12), (2, 2), (16, 16), first=3, count=2)
    with pytest.raises(MI355XError):
        ops.tile_gather(torch.zeros(1, 3, 32, 28), (0, 0), (12, 12), (2, 2), (16, 16))


def _bf(P):
    return {k: (v.to(torch.bfloat16).float() if v.dim() > 1 else v) for k, v in P.items()}


@pytest.fixture(scope="module")
def mini():
    from paddlemix_amd.vae import AutoencoderKL, synth_vae_params
    P = _bf(synth_vae_params(MINI_VAE, seed=7))

    def make(**kw):
        vae = AutoencoderKL(MINI_VAE, P, **kw)
        vae.tile_latent_min_size, vae.tile_sample_min_size = 16, 64
        vae.enable_tiling()
        return vae
    return P, make


@pytest.mark.parametrize("shape", [(2, 4, 32, 28), (2, 4, 32, 25)])
def test_mini_vae_tiled_decode(mini, shape):
    P, make = mini
    z = torch.randn(*shape, generator=torch.Generator().manual_seed(1))
    ref = TR.tiled_decode(P, MINI_VAE, z, 16, 64)
    vae = make()
    out = vae.decode(z.cuda()).sample
    r = _rel(out.cpu(), ref)
    print(f"mini-vae tiled decode {shape}: rel-L2 vs restatement {r:.3e}")
    assert out.shape == ref.shape and r <= 2e-2, r
    assert torch.equal(vae.decode(z.cuda()).sample, out)                       # graph replay
    assert torch.equal(make(use_graph=False).decode(z.cuda()).sample, out)
    if shape[3] == 28:
        scaled = vae.decode(z.cuda(), in_scale=1 / MINI_VAE["scaling_factor"]).sample
        assert _rel(scaled.cpu(), TR.tiled_decode(P, MINI_VAE, z, 16, 64, scaled=True)) <= 2e-2
        vae.enable_slicing()
        assert _rel(vae.decode(z.cuda()).sample.cpu(), ref) <= 2e-2


def test_mini_vae_tiled_encode(mini):
    P, make = mini
    g = torch.Generator().manual_seed(6)
    x = torch.rand(2, 3, 128, 112, generator=g) * 2 - 1
    noise = torch.randn(2, 4, 32, 28, generator=g)
    mean, logvar, sample = TR.tiled_encode(P, MINI_VAE, x, 16, 64, noise=noise)
    vae = make()
    post = vae.encode(x.cuda()).latent_dist
    r = (_rel(post.mean.cpu(), mean), _rel(post.logvar.cpu(), logvar), _rel(post.sample(noise=noise.cuda()).cpu(), sample))
    print("mini-vae tiled encode: rel-L2 vs restatement (mean, logvar, sample) = %.3e %.3e %.3e" % r)
    assert post.mean.shape == mean.shape and max(r) <= 2e-2, r
    again = vae.encode(x.cuda()).latent_dist
    assert torch.equal(again.mean, post.mean) and torch.equal(again.logvar, post.logvar)
    assert torch.equal(make(use_graph=False).encode(x.cuda()).latent_dist.mean, post.mean)


def test_sd_vae_tiled_decode_four_tiles():
    """the full SD decoder on four tiles of <= 256 px: z [1, 4, 40, 32] with 32-latent tiles -> (1, 3, 320, 256)"""
    from paddlemix_amd.vae import AutoencoderKL, synth_decoder_params
    P = _bf(synth_decoder_params(SD_VAE, 11))
    z = torch.randn(1, 4, 40, 32, generator=torch.Generator().manual_seed(3))
    vae = AutoencoderKL(SD_VAE, P)
    vae.tile_latent_min_size, vae.tile_sample_min_size = 32, 256
    vae.enable_tiling()
    out = vae.decode(z.cuda()).sample
    ref = TR.tiled_decode(P, SD_VAE, z, 32, 256)
    r = _rel(out.cpu(), ref)
    print(f"sd-vae tiled decode 320x256: rel-L2 vs restatement {r:.3e}")
    assert out.shape == (1, 3, 320, 256) and torch.isfinite(out).all() and r <= 2e-2, r
