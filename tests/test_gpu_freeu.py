"""-m gpu: FreeU on the device (ABI 22; csrc/freeu.hip and its stage in both planners).

Kernel: mi355x_sd_freeu over the matrix of tests/freeu_child.py -- every plane size, the shape the row split engages on, aligned /
odd-Cx / tail channel layouts and one wide enough for several grid columns per span, 16-bit and fp32 elements, six input kinds -- held elementwise to the float64 bound of
tests/freeu_bounds.py on the bf16 and the fp16 build; untouched columns, padding and the rows behind the buffer bit-unchanged; two runs
bit-identical.

U-Net: TINY and MINI_XL at 2 x 4 x 16 x 16 with FreeU (s1 = 0.9, s2 = 0.2, b1 = 1.3, b2 = 1.4) against the oracle with apply_freeu
patched into its up resnets, at the tolerance of tests/test_gpu_unet.py's cases for the same configs (rel-L2 2e-2). The margin is the
oracle's own distance between its FreeU and its plain forward on the same inputs in float64, computed on the CPU: 0.455 (TINY) and
0.509 (MINI_XL) with these constants, at least 10 x the tolerance -- a product that ignored FreeU would sit at the margin, not under
the tolerance. (1, 1, 1, 1) and off-after-on are bit-identical to never on; the C handle with mi355x_sd_unet_set_freeu and an
exported program are bit-identical to the Python-planned model."""
import pytest
import torch

from oracle import unet_ref as U
from tests import freeu_bounds as FB
from tests.freeu_child import CASES, CHANNELS
from tests.gpu_child import Family

pytestmark = pytest.mark.gpu
TOL = 2e-2   # tests/test_gpu_unet.py test_small_unet_vs_oracle ("tiny", "mini-xl")
GEOM = {"tiny": ("TINY", 2, 16, 16, 7), "mini-xl": ("MINI_XL", 2, 16, 16, 77)}


KERNEL = Family("freeu_child.py", "FREEU_JSON", None, timeout=300)
UNET = Family("freeu_child.py", "FREEU_JSON", None, timeout=600)


def _kernel(dtype):
    return KERNEL.child(("kernel",), {"MI355X_SD_DTYPE": dtype})


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_case(name, dtype):
    v = _kernel(dtype)[name]
    print(f"{name:<28} {dtype} splits {v['splits']} " + " ".join(f"{k} {r:.3f}" for k, r in v["ratio"].items()))
    assert v["rc"] == 0
    assert all(r < 1.0 for r in v["ratio"].values()), v["ratio"]
    assert v["untouched_off"] == 0      # columns [Cx // 2, Cx), the row padding and the rows behind the buffer keep their bits
    assert v["rerun_off"] == 0          # two runs, the same bits
    if CASES[name][:2] == FB.SPLIT_SHAPE and CHANNELS[CASES[name][2]][1] == 64:
        assert v["splits"] > 1          # the shape named for it (at Cs = 64): the plane's rows are split over blocks


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """the oracle's forwards with and without FreeU (float32 weights as the device holds them, rounded to bf16), computed once on the
    CPU; the float64 margin between the two"""
    from paddlemix_amd.unet import synth_unet_params
    from tests import configs
    from tests.test_gpu_unet import _inputs
    out, margins = {}, {}
    for name, (cfgname, B, H, W, L) in GEOM.items():
        cfg = getattr(configs, cfgname)
        P = {k: (v.to(torch.bfloat16).float() if v.dim() > 1 else v) for k, v in synth_unet_params(cfg, seed=1234).items()}
        sample, enc, added = _inputs(cfg, B, H, W, L)
        dbl = lambda x: None if x is None else ({k: v.double() for k, v in x.items()} if isinstance(x, dict) else x.double())  # noqa: E731
        P64 = {k: v.double() for k, v in P.items()}
        off64 = U.unet_forward(P64, cfg, dbl(sample), 501, dbl(enc), added_cond_kwargs=dbl(added))
        ref_off = U.unet_forward(P, cfg, sample, 501, enc, added_cond_kwargs=added)
        with pytest.MonkeyPatch.context() as mp:
            FB.patch_oracle(mp, cfg, **FB.FREEU)
            on64 = U.unet_forward(P64, cfg, dbl(sample), 501, dbl(enc), added_cond_kwargs=dbl(added))
            ref_on = U.unet_forward(P, cfg, sample, 501, enc, added_cond_kwargs=added)
        margins[name] = ((on64 - off64).norm() / off64.norm()).item()
        out[name] = dict(cfg=cfgname, params=P, sample=sample, enc=enc, added=added, ref_on=ref_on, ref_off=ref_off)
    path = str(tmp_path_factory.mktemp("freeu") / "refs.pt")
    torch.save(out, path)
    return path, margins


def _unet(refs):
    return UNET.child(("unet", refs[0]), {"MI355X_SD_DTYPE": "bf16"})


@pytest.mark.parametrize("name", list(GEOM))
def test_unet_with_freeu_vs_patched_oracle(name, refs):
    margin = refs[1][name]
    v = _unet(refs)[name]
    print(f"{name}: margin {margin:.3f}; " + "; ".join(f"{g}: on {v[g]['rel_on']:.3e} off {v[g]['rel_off']:.3e} on-vs-plain-oracle "
                                                       f"{v[g]['rel_on_vs_off_ref']:.3f}" for g in ("eager", "graph")))
    assert margin >= 10 * TOL, margin
    for g in ("eager", "graph"):
        assert v[g]["rel_on"] < TOL and v[g]["rel_off"] < TOL, v[g]
        assert v[g]["ones_equal_off"] and v[g]["off_after_on_equal"], v[g]     # (1, 1, 1, 1) and off-after-on: the bits of never on
        assert v[g]["plans"] == 3
    assert v["graph_equals_eager"]


def test_c_handle_equals_python_planned_model(refs):
    c = _unet(refs)["tiny"]["cexec"]
    assert c["on_equal"] and c["off_equal"] and c["off_after_on_equal"], c


def test_exported_program_replays_like_the_live_model(refs):
    e = _unet(refs)["tiny"]["export"]
    assert e["freeu_launches"] == 6 and e["live_is_on"] and e["replay_equal"], e
