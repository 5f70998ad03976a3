"""Run the REFERENCE's own EulerAncestralDiscreteScheduler (schedulers/scheduling_euler_ancestral_discrete.py, unmodified, from
/root/reference) over oracle/paddle_shim.py through the toy loops of tests/euler_ancestral_cases.py and store its timesteps, sigmas,
init_noise_sigma, the per-step noise and the end latents under tests/golden/euler_ancestral/<case>.npz (fp32). The reference draws
its noise through its module-level ``randn_tensor``; that attribute is replaced here, at run time, by a function that hands out the
pre-drawn planes of the case (no file of the reference or of oracle/ is edited).

    python scripts/make_euler_ancestral_golden.py [case ...]        (build container only; CPU, seconds)

For every case it also prints the reference's own float32-against-float64 difference (the same loop on float64 tensors: the
reference casts its sigmas to the model output's dtype) and the product class's difference from the reference.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import reference_runner as rr  # noqa: E402
from tests import euler_ancestral_cases as EC  # noqa: E402

if not rr.available():
    sys.exit("/root/reference is not present: the golden vectors can only be regenerated in the build container")
mod = rr.ref_module("scheduling_euler_ancestral_discrete", "schedulers")
ref = mod.EulerAncestralDiscreteScheduler

from paddlemix_amd.schedulers import EulerAncestralDiscreteScheduler  # noqa: E402


def ref_step(sch, eps, t, x, z):
    """the reference's step() with its randn_tensor returning z (checked: called exactly once, for the model output's shape)"""
    handed = []

    def randn_tensor(shape, generator=None, dtype=None, **_):
        assert list(shape) == list(rr.from_shim(z).shape) and not handed
        handed.append(1)
        return z
    mod.randn_tensor = randn_tensor
    out = sch.step(eps, t, x, return_dict=False)[0]
    assert handed, "the reference drew no noise"
    return out


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


os.makedirs(EC.GOLDEN_DIR, exist_ok=True)
for name in sys.argv[1:] or list(EC.CONFIGS):
    kw, steps, first = EC.CONFIGS[name]
    lat, ts, sig, s0, zs = EC.toy_loop(ref(**kw), steps, first, wrap=rr.to_shim, unwrap=rr.from_shim, step=ref_step)
    assert torch.isfinite(lat).all() and lat.dtype == torch.float32, name
    np.savez(EC.golden_path(name), latents=lat.numpy(), timesteps=np.asarray(ts, dtype=np.float32), sigmas=np.asarray(sig, dtype=np.float32),
             init_noise_sigma=np.float32(s0), noise=zs.numpy())
    try:
        lat64 = EC.toy_loop(ref(**kw), steps, first, dtype=torch.float64, wrap=rr.to_shim, unwrap=rr.from_shim, step=ref_step)[0]
        f64 = f"{rel(lat, lat64):.3g} ({lat64.dtype})"
    except Exception as ex:   # noqa: BLE001  (information only)
        f64 = f"not run ({type(ex).__name__}: {ex})"
    own, own_ts, own_sig, own_s0, _ = EC.toy_loop(EulerAncestralDiscreteScheduler(**kw), steps, first)
    print(f"{name:20s} {steps:2d} steps from {first}: reference fp32 vs fp64 {f64}; product vs reference {rel(own, lat):.3g}, "
          f"timesteps {max(abs(a - b) for a, b in zip(own_ts, ts)):.3g}, sigmas {max(abs(a - b) for a, b in zip(own_sig, sig)):.3g}, "
          f"init_noise_sigma {abs(own_s0 - s0):.3g}", flush=True)
