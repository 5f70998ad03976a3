"""-m gpu: the T2I-Adapter on the device (ABI 23; csrc/adapter.hip, paddlemix_amd/adapter.py, the intrablock adds of the U-Net plan).

Kernels (tests/adapter_child.py, on the bf16 and the fp16 build):
  pixel-unshuffle  exact bits against torch.pixel_unshuffle(x, r).permute(0, 2, 3, 1) cast to the element type; padded rows untouched
  average pool     the float64 pool of the stored inputs, e = 3 * 2^-24 * the window's mean |x| (an fp32 sum of at most four terms and
                   an exact scale: derived, not measured), through tests/bound_pieces.check; even, odd, single-pixel, odd x even sizes
  ReLU             equal in value to torch.relu on finite inputs with +-0, the smallest and the largest magnitudes; in and out of place

Models (bf16 build; references computed here on the CPU once, with the weights rounded as the device holds them):
  the three adapter types at 64 x 64 px and at 72 x 88 px (latent 9 x 11 -> 5 x 6 -> 3 x 3 -> 2 x 2: every pool is a ceil-mode one) against
  tests/adapter_ref.adapter_forward, at the rel-L2 the ControlNet parity test of tests/test_gpu_unet.py holds its residuals to (2e-2);
  the fp16 build at tests/test_gpu_fp16.py's whole-model bar (3e-3);
  the U-Net with intrablock residuals on the SD-1.5-shaped and the SDXL-shaped miniature against unet_forward_intrablock at the
  tolerance of tests/test_gpu_unet.py for these sizes (2e-2): zero residuals give the plain bits, the deprecated argument the
  intrablock bits, an odd latent with the adapter's own features meets the U-Net's shapes; one 4-step pipeline call."""
import pytest
import torch

from tests import adapter_cases as AC
from tests import adapter_ref as AR
from tests.adapter_child import AVGPOOL, RELU, UNSHUFFLE
from tests.gpu_child import Family

pytestmark = pytest.mark.gpu
TOL = {"bf16": 2e-2, "fp16": 3e-3}   # tests/test_gpu_unet.py (ControlNet residuals, small U-Nets); tests/test_gpu_fp16.py (whole models)
FAMILY = Family("adapter_child.py", "ADAPTER_JSON", None, timeout=600)
GEOMS = [("full", 64, 64), ("full", 72, 88), ("xl", 64, 64), ("xl-r8", 72, 88), ("light", 64, 64), ("light", 72, 88)]


def _kernel(dtype):
    return FAMILY.child(("kernel",), {"MI355X_SD_DTYPE": dtype})


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(UNSHUFFLE))
def test_pixel_unshuffle_exact_bits(name, dtype):
    v = _kernel(dtype)["unshuffle"][name]
    assert v["off"] == 0 and v["untouched_off"] == 0, v


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(AVGPOOL))
def test_avgpool2_within_the_float64_bound(name, dtype):
    v = _kernel(dtype)["avgpool"][name]
    print(f"{name} {dtype}: {v['ratio']:.3f} of the bound, rel-L2 {v['rel']:.2e}")
    B, H, W, C, _ = AVGPOOL[name]
    assert v["shape"] == [(H + 1) // 2, (W + 1) // 2] and v["ratio"] < 1.0 and v["untouched_off"] == 0, v


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(RELU))
def test_relu_equals_torch(name, dtype):
    v = _kernel(dtype)["relu"][name]
    assert v["unequal"] == 0 and v["untouched_off"] == 0 and v["input_off"] == 0, v


def _adapter_config(name):
    return dict(AR.ADAPTERS["xl"], downscale_factor=8) if name == "xl-r8" else AR.ADAPTERS[name]


def _refs(tmp_path_factory, dtype):
    """everything the model child compares with, computed once on the CPU"""
    from paddlemix_amd.unet import synth_unet_params
    et = torch.bfloat16 if dtype == "bf16" else torch.float16
    out = {"adapter": {}, "unet": {}}
    for name, H, W in GEOMS:
        config = _adapter_config(name)
        P = AC.rounded(AR.synth_adapter_params(config, seed=21), et)
        x = AC.image(2, config["in_channels"], H, W)
        out["adapter"][f"{name}-{H}x{W}"] = dict(config=config, params=P, image=x, ref=AR.adapter_forward(P, config, x))
    if dtype == "bf16":
        for name, (cfg, adapter, up, L) in AC.UNETS.items():
            P = AC.rounded(synth_unet_params(cfg, seed=1234))
            B, H, W = 2, 16, 16
            sample, enc, added = AC.unet_inputs(cfg, B, H, W, L)
            res = AC.residuals(cfg, B, H, W)
            r = dict(cfg=cfg, params=P, sample=sample, enc=enc, added=added, residuals=res,
                     ref_plain=AR.U.unet_forward(P, cfg, sample, 501, enc, added_cond_kwargs=added),
                     ref_on=AR.unet_forward_intrablock(P, cfg, sample, 501, enc, down_intrablock_additional_residuals=res,
                                                       added_cond_kwargs=added))
            aconfig = _adapter_config("xl-r8" if adapter == "xl" else adapter)
            AP = AC.rounded(AR.synth_adapter_params(aconfig, seed=21))
            img = AC.image(B, aconfig["in_channels"], 72, 88)
            feats = AR.adapter_forward(AP, aconfig, img)
            s2, e2, a2 = AC.unet_inputs(cfg, B, 9 * up, 11 * up, L, seed=3)
            r["odd"] = dict(adapter_config=aconfig, adapter_params=AP, image=img, sample=s2, enc=e2, added=a2,
                            ref=AR.unet_forward_intrablock(P, cfg, s2, 501, e2, down_intrablock_additional_residuals=feats,
                                                           added_cond_kwargs=a2))
            out["unet"][name] = r
        g = torch.Generator().manual_seed(0)
        out["pipeline"] = dict(pe=torch.randn(1, 7, 64, generator=g), ne=torch.randn(1, 7, 64, generator=g),
                               lat0=torch.randn(1, 4, 9, 11, generator=g), image=AC.image(1, 3, 72, 88))
    path = str(tmp_path_factory.mktemp("adapter") / f"refs_{dtype}.pt")
    torch.save(out, path)
    return path


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    made = {}
    return lambda dtype: made.setdefault(dtype, _refs(tmp_path_factory, dtype))


def _model(refs, dtype):
    return FAMILY.child(("model" if dtype == "bf16" else "adapters", refs(dtype)), {"MI355X_SD_DTYPE": dtype})


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name,H,W", GEOMS)
def test_adapter_forward_vs_restatement(name, H, W, dtype, refs):
    v = _model(refs, dtype)["adapter"][f"{name}-{H}x{W}"]
    print(f"{name} {H}x{W} {dtype}: rel-L2 per feature " + " ".join(f"{r:.2e}" for r in v["rel"]))
    assert len(v["rel"]) == v["n_ref"] and v["fp32"] and v["rerun_equal"]
    assert max(v["rel"]) < TOL[dtype], v["rel"]
    if (name, H, W) == ("full", 72, 88):
        assert v["shapes"] == [list(s) for s in AR.intrablock_shapes(AC.MINI_SD15, 2, 9, 11)[:4]]


@pytest.mark.parametrize("name", list(AC.UNETS))
def test_unet_with_intrablock_residuals(name, refs):
    v = _model(refs, "bf16")["unet"][name]
    for g in ("eager", "graph"):
        r = v[g]
        print(f"{name} {g}: with residuals {r['rel_on']:.3e}, plain {r['rel_plain']:.3e} vs the restatement; the residuals move it by {r['on_vs_plain']:.3f}")
        assert r["zero_equals_plain"], "(i) x + 0 is exact: zero residuals must give the plain forward's bits"
        assert r["deprecated_equals_intrablock"], "(ii) the deprecated argument is the intrablock form"
        assert r["rel_on"] < TOL["bf16"] and r["rel_plain"] < TOL["bf16"], r                     # (iii)
        assert r["on_vs_plain"] > 10 * TOL["bf16"], "O(1) residuals move the prediction by far more than the tolerance"
        assert r["plain_after_equals_plain"] and r["plans"] == 2
    assert v["graph_equals_eager"]
    o = v["odd"]                                                                                  # (iv)
    print(f"{name} odd latent: {o['rel']:.3e}, features {o['feature_shapes']}")
    up = AC.UNETS[name][2]
    assert o["feature_shapes"] == [list(s) for s in AR.intrablock_shapes(AC.UNETS[name][0], 2, 9 * up, 11 * up)[:4]]
    assert o["adds"] == 4 and o["rel"] < TOL["bf16"], o


def test_pipeline_smoke(refs):
    p = _model(refs, "bf16")["pipeline"]
    assert p["finite"] and p["on_vs_plain"] > 1e-2 and p["factor0_equals_plain"], p
