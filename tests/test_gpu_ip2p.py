"""-m gpu: InstructPix2Pix on the device (ABI 24; csrc/ip2p.hip and the loop of paddlemix_amd/pipeline.py).

Kernels, on the bf16 and the fp16 build (the kernels are fp32; both builds compile them): mi355x_sd_guidance3 over the matrices of
tests/ip2p_cases.py, every element inside the float64 bound of tests/ip2p_bounds.py on inputs whose three terms cancel to 1e-3 in a
tenth of the elements (flat form) and that carry a common offset of 50 (rescale forms: per_sample 2, 396 and both sides of the
32768 at which a sample stops being register-resident; sigma 14.6 and 0.03 for the x0 form); the padding around out and the inputs keep
their bits; two runs are bit-identical. mi355x_sd_ip2p_input is held to the bits of the torch expression it replaces.

Loop, bf16 build, the miniature SD-1.5-shaped and SDXL-shaped 8-channel U-Nets at 2 x 16 x 16, 4 steps, Euler a and DPM-Solver
multistep. Every loop, fused and fused_update=False, live on the device U-Net, is compared with the restatement (tests/ip2p_ref.py)
run on the CPU around the oracle U-Net at the rel-L2 tests/test_gpu_unet.py uses for these configurations (2e-2); Euler a's
restatement takes the per-step draws of the same seeded device generator, copied to the host, through ``step``'s ``noise=``.
image_guidance_scale 1.0 against 2.5 moves the result by more than ten times that.

Fused against fused_update=False, and against the torch-op restatement on the device, on the U-Net outputs the fused loop recorded:
rtol = atol = 2e-5. This is NOT a derived per-step bound: it is the tolerance tests/test_fused_vpred.py and tests/test_ip2p_host.py
use for the same pair of loops, borrowed. What is derived is held per step on the emulator (tests/test_ip2p_host.py: the guided
output against the float64 reference within tests/ip2p_bounds.py) and, for each tail against its float64 step, in that tail's own
family (tests/test_gpu_ancestral.py, tests/test_gpu_multistep.py); the tails are unchanged here and run with eps_text == NULL.

In place of the issue's "text2img on the same U-Net gives the same bits before and after": ONE PLAIN FORWARD of the same U-Net
before and after an InstructPix2Pix call. The issue's check cannot be run as stated: an 8-channel U-Net with 4 output channels has no
text2img loop, whose step needs the model output in the latents' shape. The text2img launch list and bits before and after are
checked on the emulator with a separate 4-channel U-Net (tests/test_ip2p_host.py)."""
import pytest
import torch

from oracle import unet_ref as U
from tests import ip2p_cases as C
from tests import ip2p_ref as R
from tests.gpu_child import Family

pytestmark = pytest.mark.gpu
TOL = 2e-2   # tests/test_gpu_unet.py test_small_unet_vs_oracle ("tiny", "mini-xl")
KERNEL = Family("ip2p_child.py", "IP2P_JSON", None, timeout=300)
LOOP = Family("ip2p_child.py", "IP2P_JSON", None, timeout=600)
LOOPS = {f"{u} {s}": (u, s) for u in C.UNETS for s in ("euler_a", "dpm")}


def _kernel(dtype):
    return KERNEL.child(("kernel",), {"MI355X_SD_DTYPE": dtype})


def _held(v):
    assert v["padding_off"] == 0 and v["inputs_off"] == 0, v      # the canaries around every buffer, and everything read


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(C.FLAT))
def test_guidance3_flat(name, dtype):
    v = _kernel(dtype)["flat"][name]
    print(f"{name:<20} {dtype} |out - ref| / bound {v['ratio']:.3f} vector path {v['vector']}")
    assert v["ratio"] < 1.0 and v["bound_finite"] and v["rerun_off"] == 0
    assert v["vector"] == int("off4" not in name and (C.FLAT[name]["batch"] * C.FLAT[name]["n"]) % 4 == 0)
    _held(v)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(C.RESCALE))
def test_guidance3_rescale(name, dtype):
    v = _kernel(dtype)["rescale"][name]
    print(f"{name:<24} {dtype} |out - ref| / bound {v['ratio']:.3f}")
    assert v["ratio"] < 1.0 and v["bound_finite"]
    assert v["rerun_off"] == 0          # two runs, the same bits: fixed trees, no atomics
    _held(v)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(C.INPUT))
def test_ip2p_input_is_the_torch_expression_bit_for_bit(name, dtype):
    v = _kernel(dtype)["input"][name]
    assert v["off"] == 0
    _held(v)


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """the loops' inputs and weights (rounded to bf16, as the device holds them) and, for DPM-Solver multistep, the restatement's end
    latents around the oracle U-Net, computed once on the CPU (Euler a's need the device generator's draws: the child computes them)"""
    from paddlemix_amd.unet import synth_unet_params
    out = {}
    for name, (uname, sched) in LOOPS.items():
        cfg = C.UNETS[uname]
        P = {k: (v.to(torch.bfloat16).float() if v.dim() > 1 else v) for k, v in synth_unet_params(cfg, seed=1234).items()}
        inp = C.loop_inputs(cfg, batch=2, hw=16, tokens=7)
        out[name] = dict(unet=uname, sched=sched, params=P, inputs=inp)
        if sched == "dpm":
            oracle = lambda x, t, encoder_hidden_states, added_cond_kwargs, return_dict: (  # noqa: E731
                U.unet_forward(P, cfg, x, float(t), encoder_hidden_states, added_cond_kwargs=added_cond_kwargs),)
            out[name]["ref"] = R.loop(oracle, C.SCHEDULERS[sched](), *inp[:4], C.STEPS, C.GS, C.GI, added=inp[4], negative_added=inp[5])
    path = str(tmp_path_factory.mktemp("ip2p") / "refs.pt")
    torch.save(out, path)
    return path, out


@pytest.mark.parametrize("name", list(LOOPS))
def test_loop(name, refs):
    v = LOOP.child(("loop", refs[0]), {"MI355X_SD_DTYPE": "bf16"})[name]
    print(f"{name}: |fused - unfused| {v['fused_vs_unfused']:.2e} |fused - torch ops| {v['fused_vs_torch_ops']:.2e} "
          f"gi 1.0 -> 2.5 moves {v['moved']:.3f} rel-L2 vs CPU restatement fused {v['rel_fused']:.3e} unfused {v['rel_unfused']:.3e}")
    assert v["fused_vs_unfused_close"] and v["fused_vs_torch_ops_close"], v
    assert v["moved"] > 10 * TOL, v
    assert v["forward_in_place_of_text2img_equal"]   # (NOT the issue's text2img loop, which this U-Net cannot run: see the docstring)
    assert v["rel_fused"] < TOL and v["rel_unfused"] < TOL, v
