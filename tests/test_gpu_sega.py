"""-m gpu: semantic guidance on the device (ABI 25; csrc/sega.hip and the loop of paddlemix_amd/pipeline.py).

Kernel, on the bf16 and the fp16 build (the kernel is fp32; both builds compile it): mi355x_sd_sega_guidance over the matrix of
tests/sega_cases.py -- plane sizes 1 .. 65536 on both sides of the wave, the block and the vector path, 1 .. 3 concepts, thresholds
0 .. 1 and an integral rank, planes of ties, zeros, -0.0, infinities, one NaN and a common offset of 50, every step form, every
pointer 4 bytes off once. Per case:
  * v[lo], v[hi] from `stats` are the sort of the reference's fp32 |g|, bit for bit;
  * thr is within 1 ulp of the float64 lerp, the same bits where v[lo] == v[hi], NaN where the plane holds a NaN;
  * the mask the kernel's threshold gives is the reference's (torch.quantile on the CPU) on EVERY element: the inputs have no |g| within
    an ulp of an inexact threshold (asserted here and, on the CPU, in tests/test_sega_host.py), so no element is left out;
  * out and momentum sit inside the elementwise float64 bound of tests/sega_bounds.py where the reference is finite and are the same
    infinity or NaN where it is not;
  * the padding around every written buffer and every input keep their bits; a second run gives the same bits.

Loop, bf16 build, the tiny U-Net at latent 16 x 16, 4 steps, DDIM and DPM-Solver multistep, two concepts through the partial and the
all-warm regime and a cool-down, with sem_guidance: the fused loop against fused_guidance=False on the U-Net outputs the fused loop
recorded. Both are float32 loops that differ in the order of a few dozen roundings per element and step (fma against separate
products, torch's lerp): 2^-14 of the largest latent, the tolerance tests/test_sega_host.py states for the same pair on the emulator."""
import pytest

from tests import sega_cases as C
from tests.gpu_child import Family

pytestmark = pytest.mark.gpu
KERNEL = Family("sega_child.py", "SEGA_JSON", None, timeout=300)
LOOP = Family("sega_child.py", "SEGA_JSON", None, timeout=300)
LOOP_TOL = 2.0 ** -14


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(C.KERNEL))
def test_sega_guidance(name, dtype):
    v = KERNEL.child(("kernel",), {"MI355X_SD_DTYPE": dtype})[name]
    print(f"{name:<36} {dtype} |out - ref| / bound {v['ratio_out']:.3f} |momentum - ref| / bound {v['ratio_mom']:.3f} vector path {v['vector']}")
    assert v["order_off"] == 0, v                                  # v[lo], v[hi]: exact
    assert v["thr_off"] == 0, v
    assert v["near"] == 0 and v["mask_off"] == 0, v                # the share of elements left out of the mask comparison is zero
    assert v["ratio_out"] < 1.0 and v["ratio_mom"] < 1.0 and v["class_off"] == 0, v
    assert v["dead_stats_off"] == 0 and v["rerun_off"] == 0, v
    assert v["padding_off"] == 0 and v["inputs_off"] == 0, v
    assert v["vector"] == int(C.KERNEL[name]["off"] == 0 and C.KERNEL[name]["hw"] % 4 == 0)


@pytest.mark.parametrize("sched", ["ddim", "dpm"])
def test_loop_fused_against_torch_ops_on_the_device(sched):
    v = LOOP.child(("loop",), {"MI355X_SD_DTYPE": "bf16"})[sched]
    print(f"{sched}: |fused - torch ops| {v['diff']:.2e} of {v['scale']:.2f} (tolerance {LOOP_TOL * v['scale']:.2e}); the edits move the "
          f"result by {v['moved']:.2e}")
    assert v["finite"] and v["diff"] < LOOP_TOL * v["scale"], v
    assert v["moved"] > 100 * LOOP_TOL * v["scale"], v
