"""Run the REFERENCE's own DPMSolverSinglestepScheduler (schedulers/scheduling_dpmsolver_singlestep.py, unmodified, loaded by
oracle/reference_runner.py over oracle/paddle_shim.py) through the toy loops of tests/singlestep_cases.py and store their timesteps,
sigmas, order list and end latents under tests/golden/singlestep/<case>.npz (latents and sigmas fp32, the rest int64).

    python scripts/make_singlestep_golden.py [case ...]        (build container only; CPU, seconds)

No file of the reference or of oracle/ is edited. For every case it also prints the reference's own float32-against-float64
difference (the same loop on float64 tensors: the reference casts its sigmas to the model output's dtype) and the product class's
difference from the reference: end latents (relative to the largest), the number of end-latent elements whose bits differ, and
whether timesteps, sigmas and order list are equal.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import reference_runner as rr  # noqa: E402
from tests import singlestep_cases as SC  # noqa: E402

if not rr.available():
    sys.exit("the reference checkout is not present: the golden vectors can only be regenerated in the build container")
REF = rr.ref_module("scheduling_dpmsolver_singlestep", "schedulers").DPMSolverSinglestepScheduler

from paddlemix_amd.schedulers import DPMSolverSinglestepScheduler  # noqa: E402


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


os.makedirs(SC.GOLDEN_DIR, exist_ok=True)
for name in sys.argv[1:] or list(SC.CONFIGS):
    kw, steps, first = SC.CONFIGS[name]
    lat, ts, sigmas, orders = SC.toy_loop(REF(**kw), steps, first, wrap=rr.to_shim, unwrap=rr.from_shim)
    assert torch.isfinite(lat).all() and lat.dtype == torch.float32, name
    np.savez(SC.golden_path(name), latents=lat.numpy(), timesteps=np.asarray(ts, dtype=np.int64),
             sigmas=np.asarray(sigmas, dtype=np.float32), order_list=np.asarray(orders, dtype=np.int64))
    try:
        lat64 = SC.toy_loop(REF(**kw), steps, first, dtype=torch.float64, wrap=rr.to_shim, unwrap=rr.from_shim)[0]
        f64 = f"{rel(lat, lat64):.3g} ({lat64.dtype})"
    except Exception as ex:   # noqa: BLE001  (information only)
        f64 = f"not run ({type(ex).__name__}: {ex})"
    own, own_ts, own_sigmas, own_orders = SC.toy_loop(DPMSolverSinglestepScheduler(**kw), steps, first)
    bits = int((own.view(torch.int32) != lat.view(torch.int32)).sum())
    print(f"{name:30s} {steps:2d} steps from {first}, orders {''.join(map(str, orders[first:]))}: reference fp32 vs fp64 {f64}; "
          f"product vs reference {rel(own, lat):.3g} ({bits} of {lat.numel()} elements differ in bits), timesteps "
          f"{'equal' if own_ts == ts else 'DIFFER'}, sigmas "
          f"{'equal' if np.array_equal(np.float32(own_sigmas), np.float32(sigmas)) else 'DIFFER'}, order list "
          f"{'equal' if own_orders == orders else 'DIFFER'}", flush=True)
