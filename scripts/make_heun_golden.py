"""Run the REFERENCE's own HeunDiscreteScheduler (schedulers/scheduling_heun_discrete.py, unmodified, loaded by
oracle/reference_runner.py over oracle/paddle_shim.py) through the toy loops of tests/heun_cases.py and store its timesteps, sigmas,
init_noise_sigma and the end latents under tests/golden/heun/<case>.npz (fp32).

    python scripts/make_heun_golden.py [case ...]        (build container only; CPU, seconds)

For every case it also prints the reference's own float32-against-float64 difference (the same loop on float64 tensors: the
reference casts its sigmas to the model output's dtype) and the product class's difference from the reference.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import reference_runner as rr  # noqa: E402
from tests import heun_cases as HC  # noqa: E402

if not rr.available():
    sys.exit("the reference checkout is not present: the golden vectors can only be regenerated in the build container")
ref = rr.ref_module("scheduling_heun_discrete", "schedulers").HeunDiscreteScheduler

from paddlemix_amd.schedulers import HeunDiscreteScheduler  # noqa: E402


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


os.makedirs(HC.GOLDEN_DIR, exist_ok=True)
for name in sys.argv[1:] or list(HC.CONFIGS):
    kw, steps, first = HC.CONFIGS[name]
    lat, ts, sig, s0 = HC.toy_loop(ref(**kw), steps, first, wrap=rr.to_shim, unwrap=rr.from_shim)
    assert torch.isfinite(lat).all() and lat.dtype == torch.float32, name
    np.savez(HC.golden_path(name), latents=lat.numpy(), timesteps=np.asarray(ts, dtype=np.float32), sigmas=np.asarray(sig, dtype=np.float32),
             init_noise_sigma=np.float32(s0))
    try:
        lat64 = HC.toy_loop(ref(**kw), steps, first, dtype=torch.float64, wrap=rr.to_shim, unwrap=rr.from_shim)[0]
        f64 = f"{rel(lat, lat64):.3g} ({lat64.dtype})"
    except Exception as ex:   # noqa: BLE001  (information only)
        f64 = f"not run ({type(ex).__name__}: {ex})"
    own, own_ts, own_sig, own_s0 = HC.toy_loop(HeunDiscreteScheduler(**kw), steps, first)
    print(f"{name:22s} {steps:2d} steps from {first}: reference fp32 vs fp64 {f64}; product vs reference {rel(own, lat):.3g}, "
          f"timesteps {max(abs(a - b) for a, b in zip(own_ts, ts)):.3g}, sigmas {max(abs(a - b) for a, b in zip(own_sig, sig)):.3g}, "
          f"init_noise_sigma {abs(np.float32(own_s0) - np.float32(s0)):.3g}", flush=True)
