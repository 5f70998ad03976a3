"""Run the REFERENCE's own UniPCMultistepScheduler (schedulers/scheduling_unipc_multistep.py, unmodified, from /root/reference) over
oracle/paddle_shim.py through the toy loops of tests/unipc_cases.py and store its timesteps and end latents under
tests/golden/unipc/<case>.npz (fp32). The shim has neither `expm1` nor `linalg.solve`; both are supplied here, at run time, as the
torch functions of the same name (the shim itself is not edited).

    python scripts/make_unipc_golden.py [case ...]        (build container only; CPU, seconds)

For every case it also prints the reference's own float32-against-float64 difference (the same loop on float64 tensors: the
reference casts its sigmas to the model output's dtype) and the product class's difference from the reference.
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import paddle_shim as PS  # noqa: E402
from oracle import reference_runner as rr  # noqa: E402
from tests import unipc_cases as UC  # noqa: E402

if not rr.available():
    sys.exit("/root/reference is not present: the golden vectors can only be regenerated in the build container")
if not hasattr(PS, "expm1"):
    PS.expm1 = PS._unary(torch.expm1)
if not hasattr(PS, "linalg"):
    PS.linalg = types.SimpleNamespace(solve=lambda a, b: PS._w(torch.linalg.solve(PS._u(a), PS._u(b))))
ref = rr.ref_module("scheduling_unipc_multistep", "schedulers").UniPCMultistepScheduler

from paddlemix_amd.schedulers import UniPCMultistepScheduler  # noqa: E402


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


os.makedirs(UC.GOLDEN_DIR, exist_ok=True)
for name in sys.argv[1:] or list(UC.CONFIGS):
    kw, steps, first = UC.CONFIGS[name]
    lat, ts = UC.toy_loop(ref(**UC.SD, **kw), steps, first, wrap=rr.to_shim, unwrap=rr.from_shim)
    assert torch.isfinite(lat).all(), name
    np.savez(UC.golden_path(name), latents=lat.float().numpy(), timesteps=np.asarray(ts, dtype=np.float32))
    try:
        lat64, _ = UC.toy_loop(ref(**UC.SD, **kw), steps, first, dtype=torch.float64, wrap=rr.to_shim, unwrap=rr.from_shim)
        f64 = f"{rel(lat, lat64):.3g} ({lat64.dtype})"
    except Exception as ex:   # noqa: BLE001  (information only)
        f64 = f"not run ({type(ex).__name__}: {ex})"
    own, own_ts = UC.toy_loop(UniPCMultistepScheduler(**UC.SD, **kw), steps, first)
    print(f"{name:30s} {steps:2d} steps from {first}: reference fp32 vs fp64 {f64}; product vs reference {rel(own, lat):.3g}, "
          f"timesteps {max(abs(a - b) for a, b in zip(own_ts, ts)):.3g}", flush=True)
