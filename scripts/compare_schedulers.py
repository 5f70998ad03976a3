#!/usr/bin/env python
"""paddlemix_amd/schedulers.py against an older copy of itself, bit for bit and in host time, in one process.

    git show <commit>:paddlemix_amd/schedulers.py > /tmp/schedulers_old.py
    python scripts/compare_schedulers.py /tmp/schedulers_old.py [--class NAME ...] [--no-grid] [--no-time]

The older file is loaded as a second module beside the current one, so library versions and CPU code paths cancel; that is why this
is a script and not a committed table of hashes. Both walk the same grid -- every class; its spacings, beta schedules, prediction
types, Karras sigmas, ``steps_offset`` and solver options; 1, 2, 3, 7, 20 and 50 steps -- and everything either produces is compared
by its bytes with dtype and shape, or by ``float.hex``, never by closeness: the freshly constructed state, the state after
``set_timesteps``, the full walk of the ``*_coefficients`` with ``model_input_scale`` and the state ``coefficient_walk`` restores,
whole ``step`` loops on seeded inputs in float32 and float64 from index 0 and from inside the schedule (with ``scale_model_input`` at
every step and ``add_noise`` before and after), and for every refusal the scheduler tests list the exception type and message. An
operation that raises is compared by what it raises. Exit status 1 at the first difference, which is named.

Then host time, old against new: ``set_timesteps`` plus one ``*_coefficients`` walk, and ``StableDiffusionDenoiser._fused_plan`` on the
emulated backend of the CPU tests, for each class's Stable Diffusion default at 20 and 50 steps; medians of interleaved repeats, with
the older module timed twice for the run-to-run spread."""
import argparse
import importlib.util
import itertools
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import paddlemix_amd.schedulers as NEW   # noqa: E402

STEPS = (1, 2, 3, 7, 20, 50)
COMMON = dict(timestep_spacing=("linspace", "leading", "trailing"), beta_schedule=("linear", "scaled_linear"), steps_offset=(0, 1))
EPS_V, ALL3, KARRAS = ("epsilon", "v_prediction"), ("epsilon", "sample", "v_prediction"), (False, True)
GRID = {   # class -> its own options (beside COMMON), the name of its coefficient method, whether step takes a generator
    "DDIMScheduler": (dict(prediction_type=ALL3, clip_sample=(False, True), set_alpha_to_one=(True, False)), "step_coefficients", True),
    "PNDMScheduler": (dict(prediction_type=EPS_V, skip_prk_steps=(True, False), set_alpha_to_one=(False, True)), "plms_coefficients", False),
    "EulerDiscreteScheduler": (dict(prediction_type=ALL3, use_karras_sigmas=KARRAS, interpolation_type=("linear", "log_linear")),
                               "step_coefficients", True),
    "EulerAncestralDiscreteScheduler": (dict(prediction_type=EPS_V), "ancestral_coefficients", True),
    "HeunDiscreteScheduler": (dict(prediction_type=ALL3, use_karras_sigmas=KARRAS, clip_sample=(False, True)), "heun_coefficients", False),
    "KDPM2DiscreteScheduler": (dict(prediction_type=EPS_V, use_karras_sigmas=KARRAS), "dpm2_coefficients", False),
    "KDPM2AncestralDiscreteScheduler": (dict(prediction_type=EPS_V, use_karras_sigmas=KARRAS), "dpm2_coefficients", True),
    "DPMSolverMultistepScheduler": (dict(prediction_type=ALL3, use_karras_sigmas=KARRAS, algorithm_type=("dpmsolver++", "dpmsolver"),
                                         solver_type=("midpoint", "heun"), solver_order=(1, 2), euler_at_final=(False, True)),
                                    "multistep_coefficients", False),
    "UniPCMultistepScheduler": (dict(prediction_type=ALL3, use_karras_sigmas=KARRAS, solver_type=("bh1", "bh2"), solver_order=(1, 2, 3),
                                     predict_x0=(True, False), lower_order_final=(True, False)), "unipc_coefficients", False),
    "LCMScheduler": (dict(prediction_type=ALL3, clip_sample=(False, True), set_alpha_to_one=(True, False)), None, True),
}
SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SD_DEFAULT = {"DDIMScheduler": dict(SD, clip_sample=False, steps_offset=1), "PNDMScheduler": dict(SD, skip_prk_steps=True, steps_offset=1),
              "LCMScheduler": dict(SD)}

GAINED_STEP_INDEX = ("DDIMScheduler", "PNDMScheduler")   # no ``step_index`` before the shared base gave every class the property

compared = 0


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod   # (dataclass-free, but keep pickling and class reprs sane)
    spec.loader.exec_module(mod)
    return mod


def enc(v, names):
    """a value as something `==` compares exactly: bytes with dtype and shape, float.hex, or structure of those"""
    global compared
    if torch.is_tensor(v):
        compared += v.numel()
        return ("tensor", str(v.dtype), tuple(v.shape), v.detach().contiguous().numpy().tobytes())
    if isinstance(v, np.ndarray):
        compared += v.size
        return ("ndarray", v.dtype.str, v.shape, v.tobytes())
    if isinstance(v, np.generic):
        compared += 1
        return ("numpy", v.dtype.str, v.tobytes())
    if isinstance(v, float):
        compared += 1
        return ("float", v.hex())
    if isinstance(v, (bool, int, str, type(None))):
        compared += 1
        return (type(v).__name__, v)
    if isinstance(v, (list, tuple)):
        return (type(v).__name__,) + tuple(enc(x, names) for x in v)
    if isinstance(v, dict):
        return ("dict",) + tuple((enc(k, names), enc(x, names)) for k, x in sorted(v.items(), key=lambda kv: repr(kv[0])))
    if isinstance(v, SimpleNamespace):
        return ("namespace", enc(vars(v), names))
    if isinstance(v, BaseException):
        compared += 1
        msg = str(v)
        for n in names:   # a message that prints the class prints its module
            msg = msg.replace(n, "<module>")
        return ("raises", type(v).__name__, msg)
    compared += 1
    return ("object", type(v).__name__)   # the walk's placeholder, a Generator


def attempt(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except Exception as e:   # compared like a value
        return e


def state(s):
    return dict(vars(s))


def seeded(shape, dtype, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype)


def loop(s, n, dtype, inside, takes_generator, **step_kw):
    """one whole loop -> everything it produced, in order"""
    out = [attempt(s.set_timesteps, n)]
    if isinstance(out[0], Exception):
        return out
    ts = s.timesteps
    start = len(ts) // 2 if inside else 0
    x, noise = seeded((2, 3), dtype, 1), seeded((2, 3), dtype, 2)
    at = torch.as_tensor(np.asarray(ts[start:start + 1]))
    out.append(attempt(s.add_noise, x, noise, at))
    if inside and not isinstance(out[-1], Exception):
        x = out[-1]
    if takes_generator:
        step_kw = dict(step_kw, generator=torch.Generator().manual_seed(3))
    for k, t in enumerate(ts[start:]):
        e = seeded((2, 3), dtype, 100 + k)
        out.append(attempt(s.scale_model_input, x, t))
        r = attempt(s.step, e, t, x, **step_kw)
        out.append(r if isinstance(r, Exception) else vars(r))
        if isinstance(r, Exception):
            break
        x = r.prev_sample
    out += [attempt(s.add_noise, x, noise, at), state(s)]
    return out


def walk(s, n, method):
    out = [attempt(s.set_timesteps, n)]
    if isinstance(out[0], Exception):
        return out
    out += [state(s), attempt(lambda: s.init_noise_sigma), s.num_inference_steps, attempt(len, s)]
    if type(s).__name__ not in GAINED_STEP_INDEX:
        out.append(s.step_index)
    if method is None:
        return out

    def rows():
        for t in s.timesteps:
            if hasattr(s, "model_input_scale"):
                out.append(s.model_input_scale(t))
            out.append(getattr(s, method)(t))

    if hasattr(s, "coefficient_walk"):
        with s.coefficient_walk():
            out.append(attempt(rows))
            out.append(state(s))   # the walked state, placeholders included
    else:
        out.append(attempt(rows))
    out.append(state(s))   # what the walk put back
    # and from inside the schedule, as an img2img loop tabulates its rows
    ts, s2 = s.timesteps, s
    if hasattr(s2, "coefficient_walk") and len(ts) > 1:
        with s2.coefficient_walk():
            out.append(attempt(lambda: [getattr(s2, method)(t) for t in ts[len(ts) // 2:]]))
        out.append(state(s2))
    return out


def one_config(mods, cls, kw, method, takes_generator):
    def both(what, fn):
        a, b = (enc(fn(getattr(m, cls)), NAMES) for m in mods)
        if a != b:
            where = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None) if isinstance(a, tuple) else None
            print(f"DIFFERENCE: {cls}({kw}) {what}: entry {where} of the record\n  old: {str(a[where] if where is not None else a)[:600]}"
                  f"\n  new: {str(b[where] if where is not None else b)[:600]}")
            sys.exit(1)

    both("fresh state", lambda C: attempt(lambda: state(C(**kw))))
    if isinstance(attempt(lambda: getattr(mods[0], cls)(**kw)), Exception):
        return
    for n in STEPS:
        both(f"set_timesteps({n}) and the coefficient walk", lambda C: walk(C(**kw), n, method))
        for dtype, inside in itertools.product((torch.float32, torch.float64), (False, True)):
            both(f"step loop n={n} {dtype} inside={inside}", lambda C: loop(C(**kw), n, dtype, inside, takes_generator))
    if cls == "DDIMScheduler":
        both("eta > 0", lambda C: loop(C(**kw), 7, torch.float32, False, True, eta=0.5, use_clipped_model_output=True))
    if cls == "EulerDiscreteScheduler":
        both("s_churn > 0", lambda C: loop(C(**kw), 7, torch.float32, False, True, s_churn=1.0))
    if cls == "LCMScheduler":
        both("custom timesteps", lambda C: [attempt((s := C(**kw)).set_timesteps, timesteps=[999, 499, 259]), state(s),
                                            attempt(s.set_timesteps, 4, strength=0.5), state(s)])


def refusals(mods):
    """every refusal of the scheduler tests' test_refusals (and the pytest.raises of tests/test_schedulers.py and
    tests/test_plms_coefficients.py): the exception type and message"""
    x = torch.ones(1, 4)

    def made(C, n=4, **kw):
        s = C(**kw)
        s.set_timesteps(n)
        return s

    def plms_stepped(M):
        s = made(M.PNDMScheduler, 5, **SD_DEFAULT["PNDMScheduler"])
        s.step(x, s.timesteps[0], x)
        return s

    def plms_zero_alpha(M):
        s = made(M.PNDMScheduler, 10, **SD_DEFAULT["PNDMScheduler"])
        s.alphas_cumprod = s.alphas_cumprod.copy()
        s.alphas_cumprod[int(s.timesteps[0])] = 0.0
        return s

    cases = []
    for cls, coef in (("HeunDiscreteScheduler", "heun_coefficients"), ("KDPM2DiscreteScheduler", "dpm2_coefficients"),
                      ("KDPM2AncestralDiscreteScheduler", "dpm2_coefficients"), ("EulerAncestralDiscreteScheduler", "ancestral_coefficients")):
        cases += [(f"{cls} trained_betas", lambda M, c=cls: getattr(M, c)(trained_betas=[0.1, 0.2])),
                  (f"{cls} squaredcos_cap_v2", lambda M, c=cls: getattr(M, c)(beta_schedule="squaredcos_cap_v2")),
                  (f"{cls} spacing", lambda M, c=cls: getattr(M, c)(timestep_spacing="middle").set_timesteps(4))]
        for pt in ("velocity",) if cls == "HeunDiscreteScheduler" else ("velocity", "sample"):   # (Heun takes sample predictions)
            cases += [(f"{cls} {pt} step", lambda M, c=cls, pt=pt: (s := made(getattr(M, c), prediction_type=pt)).step(x, s.timesteps[0], x)),
                      (f"{cls} {pt} row", lambda M, c=cls, pt=pt, f=coef: getattr(s := made(getattr(M, c), prediction_type=pt), f)(s.timesteps[0]))]
    cases += [
        ("Heun clip_sample row", lambda M: (s := made(M.HeunDiscreteScheduler, clip_sample=True)).heun_coefficients(s.timesteps[0])),
        ("Euler a fresh step", lambda M: (s := M.EulerAncestralDiscreteScheduler()).step(x, s.timesteps[0], x)),
        ("Euler a integer timestep", lambda M: made(M.EulerAncestralDiscreteScheduler).step(x, 3, x)),
        ("Euler spacing", lambda M: M.EulerDiscreteScheduler(timestep_spacing="middle").set_timesteps(4)),
        ("Euler interpolation", lambda M: M.EulerDiscreteScheduler(interpolation_type="cubic").set_timesteps(4)),
        ("Euler velocity step", lambda M: (s := made(M.EulerDiscreteScheduler, prediction_type="velocity")).step(x, s.timesteps[0], x)),
        ("Euler sample row", lambda M: (s := made(M.EulerDiscreteScheduler, prediction_type="sample")).step_coefficients(s.timesteps[0])),
        ("DDIM spacing", lambda M: M.DDIMScheduler(timestep_spacing="middle").set_timesteps(4)),
        ("DDIM too many steps", lambda M: M.DDIMScheduler().set_timesteps(1001)),
        ("DDIM fresh step", lambda M: M.DDIMScheduler().step(x, 1, x)),
        ("DDIM clipped row", lambda M: made(M.DDIMScheduler).step_coefficients(0)),
        ("DDIM velocity step", lambda M: made(M.DDIMScheduler, prediction_type="velocity").step(x, 0, x)),
        ("PNDM spacing", lambda M: M.PNDMScheduler(timestep_spacing="middle").set_timesteps(4)),
        ("PNDM fresh step_plms", lambda M: M.PNDMScheduler().step_plms(x, 1, x)),
        ("PNDM plms before prk", lambda M: made(M.PNDMScheduler, 20).step_plms(x, 1, x)),
        ("PNDM velocity step", lambda M: (s := made(M.PNDMScheduler, skip_prk_steps=True, prediction_type="velocity")).step(x, s.timesteps[0], x)),
        ("PLMS row with prk", lambda M: (s := made(M.PNDMScheduler, 20)).plms_coefficients(s.timesteps[0])),
        ("PLMS row sample", lambda M: (s := made(M.PNDMScheduler, 20, skip_prk_steps=True, prediction_type="sample")).plms_coefficients(s.timesteps[0])),
        ("PLMS row after a step", lambda M: (s := plms_stepped(M)).plms_coefficients(s.timesteps[1])),
        ("PLMS row not finite", lambda M: (s := plms_zero_alpha(M)).plms_coefficients(s.timesteps[0])),
        ("PLMS fresh row", lambda M: M.PNDMScheduler(skip_prk_steps=True).plms_coefficients(1)),
        ("DPM-Solver sde", lambda M: M.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")),
        ("DPM-Solver order 3", lambda M: M.DPMSolverMultistepScheduler(solver_order=3)),
        ("DPM-Solver solver type", lambda M: M.DPMSolverMultistepScheduler(solver_type="bh1")),
        ("DPM-Solver beta schedule", lambda M: M.DPMSolverMultistepScheduler(beta_schedule="squaredcos_cap_v2")),
        ("DPM-Solver spacing", lambda M: M.DPMSolverMultistepScheduler(timestep_spacing="middle").set_timesteps(4)),
        ("DPM-Solver fresh step", lambda M: M.DPMSolverMultistepScheduler().step(x, 0, x)),
        ("DPM-Solver fresh row", lambda M: M.DPMSolverMultistepScheduler().multistep_coefficients(0)),
        ("DPM-Solver velocity step", lambda M: (s := made(M.DPMSolverMultistepScheduler, prediction_type="velocity")).step(x, s.timesteps[0], x)),
        ("DPM-Solver velocity row", lambda M: (s := made(M.DPMSolverMultistepScheduler, prediction_type="velocity")).multistep_coefficients(s.timesteps[0])),
        ("UniPC spacing", lambda M: M.UniPCMultistepScheduler(timestep_spacing="middle").set_timesteps(4)),
        ("UniPC fresh step", lambda M: M.UniPCMultistepScheduler().step(torch.zeros(1), 0, torch.zeros(1))),
        ("UniPC fresh row", lambda M: M.UniPCMultistepScheduler().unipc_coefficients(0)),
        ("UniPC velocity step", lambda M: (s := made(M.UniPCMultistepScheduler, prediction_type="velocity")).step(x, s.timesteps[0], x)),
        ("UniPC velocity row", lambda M: (s := made(M.UniPCMultistepScheduler, prediction_type="velocity")).unipc_coefficients(s.timesteps[0])),
        ("UniPC convert without sample", lambda M: made(M.UniPCMultistepScheduler).convert_model_output(x)),
        ("UniPC Karras order 3 last row", lambda M: [(s := made(M.UniPCMultistepScheduler, 8, use_karras_sigmas=True, solver_order=3,
                                                                 lower_order_final=False, **SD)).unipc_coefficients(t) for t in s.timesteps]),
        ("LCM descending", lambda M: M.LCMScheduler().set_timesteps(timesteps=[499, 999])),
        ("LCM too many", lambda M: M.LCMScheduler().set_timesteps(60)),
        ("LCM both", lambda M: M.LCMScheduler().set_timesteps(4, timesteps=[999])),
        ("LCM neither", lambda M: M.LCMScheduler().set_timesteps()),
        ("LCM fresh step", lambda M: M.LCMScheduler().step(x, 1, x)),
        ("LCM beta schedule", lambda M: M.LCMScheduler(beta_schedule="squaredcos_cap_v2")),
    ]
    for kw in (dict(thresholding=True), dict(solver_p=object()), dict(trained_betas=[0.1, 0.2]), dict(solver_order=4),
               dict(solver_type="bh3"), dict(beta_schedule="squaredcos_cap_v2")):
        cases.append((f"UniPC {kw}", lambda M, kw=kw: M.UniPCMultistepScheduler(**kw)))
    for name, fn in cases:
        a, b = (enc(attempt(fn, m), NAMES) for m in mods)
        if a != b or a[0] != "raises":
            print(f"DIFFERENCE: refusal {name!r}\n  old: {a}\n  new: {b}" if a != b else f"NOT A REFUSAL: {name!r}: {a}")
            sys.exit(1)
    return len(cases)


def timing(mods, repeats):
    """-> text. mods = (old, new); the old module is timed twice (A, B), interleaved with the new one"""
    from paddlemix_amd.pipeline import StableDiffusionDenoiser
    from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params
    from tests.abi_emulator import on_emulator
    from tests.abi_emulator_ancestral import AncestralEmulator
    from tests.abi_emulator_dpm2 import Dpm2Emulator
    from tests.abi_emulator_guidance import GuidanceEmulator
    from tests.abi_emulator_heun import HeunEmulator
    from tests.abi_emulator_plms import PlmsEmulator
    from tests.abi_emulator_unipc import UniPCEmulator
    from tests.configs import TINY
    backends = {"PNDMScheduler": PlmsEmulator, "EulerAncestralDiscreteScheduler": AncestralEmulator, "HeunDiscreteScheduler": HeunEmulator,
                "KDPM2DiscreteScheduler": Dpm2Emulator, "KDPM2AncestralDiscreteScheduler": Dpm2Emulator,
                "DPMSolverMultistepScheduler": UniPCEmulator, "UniPCMultistepScheduler": UniPCEmulator}
    params = synth_unet_params(TINY, seed=1234)
    old, new = mods
    lines = [f"host time, microseconds, median of {repeats} interleaved repeats; old A and old B are the same older module",
             f"{'class':34s} {'steps':>5s} {'what':>12s} {'old A':>9s} {'old B':>9s} {'new':>9s} {'spread':>7s} {'new/old':>7s}"]
    total = dict(a=0.0, b=0.0, n=0.0)
    for cls, (_, method, _) in GRID.items():
        for n in (20, 50):
            def schedule_and_walk(s):
                s.set_timesteps(n)
                if method is not None:
                    for t in s.timesteps:
                        getattr(s, method)(t)

            def plan(p):
                p.scheduler.set_timesteps(n)
                p._fused_plan(False, "cpu", p.scheduler.timesteps, torch.Generator())

            kw = SD_DEFAULT.get(cls, SD)
            unet = on_emulator(UNet2DConditionModel, TINY, params, backend=backends.get(cls, GuidanceEmulator)())
            for what, fn, make in (("set+walk", schedule_and_walk, lambda M: getattr(M, cls)(**kw)),
                                   ("_fused_plan", plan, lambda M: StableDiffusionDenoiser(unet, getattr(M, cls)(**kw)))):
                t = dict(a=[], b=[], n=[])
                for _ in range(repeats):
                    for key, M in (("a", old), ("n", new), ("b", old)):
                        obj = make(M)
                        t0 = time.perf_counter()
                        fn(obj)
                        t[key].append((time.perf_counter() - t0) * 1e6)
                a, b, m = (statistics.median(t[k]) for k in "abn")
                for k, v in zip("abn", (a, b, m)):
                    total[k] += v
                lines.append(f"{cls:34s} {n:5d} {what:>12s} {a:9.1f} {b:9.1f} {m:9.1f} {abs(a - b) / min(a, b):7.1%} {m / min(a, b):7.3f}")
    a, b, m = total["a"], total["b"], total["n"]
    spread = abs(a - b) / min(a, b)
    lines.append(f"{'sum of the medians':34s} {'':5s} {'':>12s} {a:9.1f} {b:9.1f} {m:9.1f} {spread:7.1%} {m / min(a, b):7.3f}")
    lines.append(f"the older module against itself: {spread:.2%}; new against the faster of the two: {m / min(a, b) - 1:+.2%}; "
                 f"new against their mean: {m / ((a + b) / 2) - 1:+.2%}")
    return "\n".join(lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old", help="an older copy of paddlemix_amd/schedulers.py")
    ap.add_argument("--class", dest="classes", action="append", help="only this class (repeatable)")
    ap.add_argument("--no-grid", action="store_true", help="the refusals and the host time alone")
    ap.add_argument("--no-time", action="store_true")
    ap.add_argument("--repeats", type=int, default=41)
    args = ap.parse_args()
    OLD = load(args.old, "schedulers_old")
    NAMES = ("schedulers_old", "paddlemix_amd.schedulers")
    mods = (OLD, NEW)
    torch.set_num_threads(1)
    for cls, (own, method, takes_generator) in GRID.items():
        if args.no_grid or (args.classes and cls not in args.classes):
            continue
        options = dict(COMMON, **own)
        before, configs, t0 = compared, 0, time.time()
        for values in itertools.product(*options.values()):
            one_config(mods, cls, dict(zip(options, values)), method, takes_generator)
            configs += 1
        print(f"{cls}: {configs} configurations x {len(STEPS)} step counts, {(compared - before) // 2} values compared, 0 differences "
              f"({time.time() - t0:.0f} s)", flush=True)
    if not args.classes:
        print(f"refusals: {refusals(mods)} cases, the same exception type and message from both")
    print(f"0 differences; {compared // 2} values compared")
    if not args.no_time:
        print(timing(mods, args.repeats))
