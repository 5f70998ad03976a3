"""-m gpu: panorama / MultiDiffusion on the device (ABI 26; csrc/panorama.hip and the loop of paddlemix_amd/pipeline.py).

Kernels, on the bf16 and the fp16 build (the kernels are fp32; both builds compile them): mi355x_sd_view_input (1 and 2 groups) and
mi355x_sd_view_merge over the matrix of tests/panorama_cases.py, each geometry at batch 1 and 2, on normal draws with a planted
-0.0 (in every view that covers one output element: the merge must give +0.0), +inf, -inf, one NaN and a channel with a common offset
of 50. Per case:
  * both outputs equal the reference's torch expressions (tests/panorama_ref.py kernel_reference) BIT FOR BIT, a NaN matching a NaN,
    on every element;
  * where some element has a count that is no power of two, the case holds elements whose sum * (1 / count) differs from sum / count
    in fp32 (counted on the CPU by the reference), so a kernel that multiplies by a reciprocal cannot pass;
  * uncovered elements are +0.0; the padding around every written buffer and every input keep their bits; a second run gives the same
    bits; the vector path is taken exactly where the alignment rule says.

Loop, bf16 build, the tiny U-Net, 4 steps at 1 x 4 x 64 x 80, circular and not, DDIM and DPM-Solver multistep, all views in one U-Net
call: (a) fused_views=True against False on the U-Net outputs the fused loop recorded: equal bits, and the torch-op path feeds the
U-Net the bits the kernel path fed it; (b) against the restatement (tests/panorama_ref.py) on the CPU around the oracle U-Net at the
rel-L2 tests/test_gpu_ip2p.py holds its loops to for the same U-Net and step count (2e-2), the value printed; (c) one view's model
output moved on the first step moves the result in every column of that view's window and in no other."""
import pytest
import torch

from oracle import unet_ref as U
from tests import configs
from tests import panorama_cases as C
from tests import panorama_ref as R
from tests.gpu_child import Family

pytestmark = pytest.mark.gpu
TOL = 2e-2   # tests/test_gpu_ip2p.py TOL (tests/test_gpu_unet.py test_small_unet_vs_oracle "tiny")
KERNEL = Family("panorama_child.py", "PANO_JSON", None, timeout=300)
LOOP = Family("panorama_child.py", "PANO_JSON", None, timeout=600)
LOOPS = {f"{s} {'circular' if c else 'plain'}": (s, c) for s in ("ddim", "dpm") for c in (False, True)}


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(C.KERNEL))
def test_view_kernels_are_the_torch_expressions_bit_for_bit(name, dtype):
    v = KERNEL.child(("kernel",), {"MI355X_SD_DTYPE": dtype})[name]
    print(f"{name:<40} {dtype} counts up to {v['max_count']}, {v['recip']} elements a reciprocal would miss, {v['uncovered']} uncovered, "
          f"vector path {v['vector']}")
    assert v["input_off"] == 0 and v["merge_off"] == 0, v
    assert v["negzero_plus"] and v["uncovered_plus_zero"], v
    assert v["recip"] > 0 or not v["odd_counts"], v
    assert v["padding_off"] == 0 and v["inputs_off"] == 0 and v["rerun_off"] == 0, v
    assert v["vector"] == C.vector_path(C.KERNEL[name]), v


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """the loops' inputs and weights (rounded to bf16, as the device holds them) and the restatement's end latents around the oracle
    U-Net, computed once on the CPU"""
    from paddlemix_amd.unet import synth_unet_params
    cfg = configs.TINY
    P = {k: (v.to(torch.bfloat16).float() if v.dim() > 1 else v) for k, v in synth_unet_params(cfg, seed=1234).items()}
    g = torch.Generator().manual_seed(7)
    pe, ne = torch.randn(1, 7, cfg["cross_attention_dim"], generator=g), torch.randn(1, 7, cfg["cross_attention_dim"], generator=g)
    lat = torch.randn(1, 4, 64, 80, generator=g)
    oracle = lambda x, t, encoder_hidden_states, return_dict: (U.unet_forward(P, cfg, x, float(t), encoder_hidden_states),)  # noqa: E731
    out = {}
    for name, (sched, circular) in LOOPS.items():
        ref = R.loop(oracle, C.SCHEDULERS[sched](), pe, ne, lat, C.STEPS, C.GS, view_batch_size=16, circular_padding=circular)
        out[name] = dict(sched=sched, circular=circular, params=P, inputs=(pe, ne, lat), ref=ref)
    path = str(tmp_path_factory.mktemp("panorama") / "refs.pt")
    torch.save(out, path)
    return path


@pytest.mark.parametrize("name", list(LOOPS))
def test_loop(name, refs):
    v = LOOP.child(("loop", refs), {"MI355X_SD_DTYPE": "bf16"})[name]
    print(f"{name}: fused_views against torch ops: {v['views_off']} elements differ, {v['unet_input_off']} U-Net input elements differ; "
          f"rel-L2 vs the CPU restatement around the oracle {v['rel']:.3e} (bar {TOL:.0e}); a moved view moves its window by at least "
          f"{v['moved_inside']:.2e} and the rest by {v['moved_outside']:.1e}; {v['unet_calls']} U-Net calls")
    assert v["finite"] and v["views_off"] == 0 and v["unet_input_off"] == 0, v
    assert v["unet_calls"] == C.STEPS, v                     # all views of a step in one call
    assert v["moved_inside"] > 0.0 and v["moved_outside"] == 0.0, v
    assert v["rel"] < TOL, v
