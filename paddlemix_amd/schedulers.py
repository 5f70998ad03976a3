"""Scheduler API surface kept for the denoising loop (plumbing, not accelerated math).

Mirrors the reference classes' public contract -- ``set_timesteps`` / ``scale_model_input`` / ``step`` /
``init_noise_sigma`` / ``timesteps`` -- for the schedulers BASELINE.json's configs use (PNDM is what the SD-1.x checkpoints ship with):
  DDIMScheduler                      ppdiffusers/ppdiffusers/schedulers/scheduling_ddim.py:131 (step :350-475)
  EulerDiscreteScheduler             scheduling_euler_discrete.py:94 (scale_model_input :216-238, step :375-478)
  FlowMatchEulerDiscreteScheduler    scheduling_flow_match_euler_discrete.py:44 (step :187-283)
  PNDMScheduler                      scheduling_pndm.py:69 (set_timesteps :178-235, step_prk :260-320, step_plms :322-395)
  DPMSolverMultistepScheduler        scheduling_dpmsolver_multistep.py:66 (deterministic variants, orders 1-2; step :802-878)
  LCMScheduler                       scheduling_lcm.py:140 (set_timesteps :330-466, step :476-566) -- 2-8 step latent-consistency sampling
  UniPCMultistepScheduler            scheduling_unipc_multistep.py:31 (predictor :438-565, corrector :567-701, step :720-804), orders 1-3
  EulerAncestralDiscreteScheduler    scheduling_euler_ancestral_discrete.py:130 (set_timesteps :210-250, step :268-363) -- "Euler a"
  HeunDiscreteScheduler              scheduling_heun_discrete.py:71 (set_timesteps :213-277, step :349-455) -- "Heun", order 2
  KDPM2DiscreteScheduler             scheduling_k_dpm_2_discrete.py:71 (set_timesteps :209-286, step :365-462) -- "DPM2", order 2
  KDPM2AncestralDiscreteScheduler    scheduling_k_dpm_2_ancestral_discrete.py:72 (set_timesteps :210-296, step :373-478) -- "DPM2 a"
  DPMSolverSinglestepScheduler       scheduling_dpmsolver_singlestep.py:75 (order list :201-233, updates :482-734, step :815-878), orders 1-3
Schedule tables are float32 numpy like the reference's float32 tensors; ``step`` works on torch tensors of any device.

For deterministic sampling every ``step`` is a linear map  prev = a*sample + b*model_output ; ``step_coefficients``
returns (a, b) -- DDIM and Euler, epsilon and v prediction -- so the latent update can run as the library's fused
``mi355x_sd_axpby`` / ``cfg_axpby`` / ``cfg_rescale_axpby`` inside a captured graph.
The DPM-Solver multistep update is linear in two tensors, the sample and the previous step's converted model output:
``DPMSolverMultistepScheduler.multistep_coefficients`` returns (p, q, A, B, D) with  m0 = p*sample + q*model_output ,
prev = A*sample + B*m0 + D*(m0 - m1)  for the library's ``mi355x_sd_multistep_update``.
The UniPC step -- corrector, then predictor -- is linear in the sample, the model output, ``last_sample`` and up to three history
entries: ``UniPCMultistepScheduler.unipc_coefficients`` returns its 12 scalars for the library's ``mi355x_sd_unipc_update``.
The ancestral Euler step is linear in the sample, the model output and the step's noise:
``EulerAncestralDiscreteScheduler.ancestral_coefficients`` returns (a, b, c) with  prev = a*sample + b*model_output + c*noise  for the
library's ``mi355x_sd_ancestral_update``; the noise stays a host draw (``torch.randn`` from the call's generator).
The Heun step has two stages, each linear in the sample, the model output and the state the first stage parks (the sample and the
derivative): ``HeunDiscreteScheduler.heun_coefficients`` returns (p, q, h, g, second) for the library's ``mi355x_sd_heun_update``.
The DPM2 step is a midpoint method of the same two-stage shape that parks the sample alone, and its ancestral variant adds noise in
the second stage: ``dpm2_coefficients`` of both classes returns (p, q, h, c, second) for the library's ``mi355x_sd_dpm2_update``.
The PLMS step (PNDM with ``skip_prk_steps``) is linear in the sample, the model output, up to three stored model outputs and one parked
sample: ``PNDMScheduler.plms_coefficients`` returns its row of 12 for the library's ``mi355x_sd_plms_update``.
The singlestep DPM-Solver evaluation is linear in the sample, the model output, the sample parked at the start of its group and the
group's first two converted outputs: ``DPMSolverSinglestepScheduler.singlestep_coefficients`` returns (p, q, A, B, E1, E2, order, keep)
for the library's ``mi355x_sd_singlestep_update``.

The schedule pieces. Every class below is put together from module-level functions that are each written once, and from one base
plus one mixin:
  _make_betas, _train_table          the training table (alphas_cumprod, sigmas) in one of two arithmetics; ``_train_table`` says why two
  _spaced_timesteps                  the linspace / leading / trailing inference timesteps; point count, rounding and dtype are arguments
  _karras_schedule, _sigma_to_t      the Karras sigma ramp and the (fractional) training timestep of each of its sigmas
  _check_prediction_type, _sigma_x0, _sigma_derivative_pq
                                     sigma space: the accepted prediction types, x0 from the model output, and the derivative
                                     (x - x0) / sigma as the linear form p*x + q*model_output
  _alpha_convert, _alpha_convert_pq, _multistep_schedule
                                     alpha space (DPM-Solver, UniPC): the converted model output, its linear form, the sigma table
  _Schedule                          base of every class with a beta schedule: config capture, the training table, ``__len__``,
                                     ``step_index``, the alpha-space ``add_noise``, the identity ``scale_model_input``, and the
                                     construction sequence, which ends in the class's ``_reset`` -- the step state that
                                     ``set_timesteps`` resets too
  _SigmaSpace                        mixin of the sigma-schedule classes (Euler, Euler a, Heun, DPM2, DPM2 a): ``_init_step_index``,
                                     ``index_for_timestep``, ``model_input_scale``, ``scale_model_input``, ``add_noise``,
                                     ``init_noise_sigma`` and ``_spaced_sigmas``, ``set_timesteps`` up to the class's table layout
A new scheduler class states its constructor signature (``self._capture(locals())`` records it), what it refuses, its table layout
in ``set_timesteps``, its ``_reset``, its ``step`` and its ``*_coefficients``. Where its arithmetic differs from a sibling's in a way
that shows in a bit of a result, that is a named class attribute or argument (``_train_arithmetic``, ``_float32_init_sigma``,
``_karras_ends_as_float``, ``_karras_rounded``, ``_spacing_hint``), never a second copy of the expression.
scripts/compare_schedulers.py walks every class over its options against an older copy of this file, bit for bit.
"""
from __future__ import annotations

from contextlib import contextmanager
from math import isfinite
from types import SimpleNamespace
from typing import Optional, Tuple

import numpy as np
import torch


def _make_betas(n: int, beta_start: float, beta_end: float, schedule: str, tensor: bool = False, who=None):
    """float32 betas: a numpy array (``np.linspace`` in float64, rounded to float32) or, with `tensor`, a torch tensor
    (``torch.linspace`` in float32). `who` names the class in the refusal, for the classes whose reference does."""
    if tensor:
        def linspace(lo, hi): return torch.linspace(lo, hi, n, dtype=torch.float32)
    else:
        def linspace(lo, hi): return np.linspace(lo, hi, n, dtype=np.float32)
    if schedule == "linear":
        return linspace(beta_start, beta_end)
    if schedule == "scaled_linear":  # the latent-diffusion schedule
        return linspace(beta_start ** 0.5, beta_end ** 0.5) ** 2
    raise NotImplementedError(f"{schedule} is not implemented" if who is None else f"{schedule} does is not implemented for {who}")


def _sigmas_of(alphas_cumprod):
    return ((1 - alphas_cumprod) / alphas_cumprod) ** 0.5


def _train_table(n: int, beta_start: float, beta_end: float, schedule: str, arithmetic: str, who=None):
    """-> (alphas_cumprod, training sigmas), float32 numpy arrays, in one of two arithmetics:
      "numpy"   ``_make_betas``' float64 linspace rounded to float32, then ``np.cumprod`` in float32: what the first classes here were
                pinned with (DDIM, PNDM, Euler, DPM-Solver, UniPC, LCM), and what their golden loops hold them to.
      "tensor"  float32 TENSOR operations throughout -- linspace, cumprod, the sigmas' division and square root -- as the reference
                builds its tables. The numpy table ends 9 float32 steps away at sigma_max (8.6e-6 at 14.6), and a loop that divides by
                sigma^2 at every step (Euler a, Heun, DPM2, DPM2 a) carries that into the latents: on ``ea_leading_offset1`` it put 2
                of 512 elements at 1.2 times the test's elementwise tolerance (tests/golden/euler_ancestral/README.md).
    A class names its choice in ``_train_arithmetic``; tests/test_schedule_pieces.py pins the choice per class."""
    if arithmetic == "tensor":
        a = torch.cumprod(1.0 - _make_betas(n, beta_start, beta_end, schedule, True, who), 0)
        return a.numpy(), _sigmas_of(a).numpy()
    if arithmetic != "numpy":
        raise ValueError(f"arithmetic {arithmetic!r}: 'numpy' or 'tensor'")
    a = np.cumprod(1.0 - _make_betas(n, beta_start, beta_end, schedule, False, who), dtype=np.float32)
    return a, _sigmas_of(a)


_SPACING_HINT = ". Please make sure to choose one of 'linspace', 'leading' or 'trailing'."


def _spaced_timesteps(spacing: str, T: int, n: int, steps_offset: int, *, dtype, round_linspace: bool = True,
                      drop_last: bool = False, hint: bool = True) -> np.ndarray:
    """The `n` inference timesteps of a `T`-step training schedule, descending, as `dtype`.
      drop_last       "linspace" and "leading" place n + 1 points and drop the lowest (DPM-Solver, UniPC); "trailing" has no such form
      round_linspace  False: the "linspace" points stay fractional (the sigma-schedule classes interpolate their sigmas at them)
      hint            whether the unsupported-spacing message names the choices (each class keeps its reference's wording)
    `steps_offset` shifts "leading" alone."""
    m = n + 1 if drop_last else n
    if spacing == "linspace":
        ts = np.linspace(0, T - 1, m)
        ts = ts.round() if round_linspace else ts
    elif spacing == "leading":
        ts = (np.arange(0, m) * (T // m)).round()
    elif spacing == "trailing":
        return np.arange(T, 0, -T / n).round().astype(dtype) - 1
    else:
        raise ValueError(f"{spacing} is not supported" + (_SPACING_HINT if hint else ""))
    ts = (ts[::-1][:-1] if drop_last else ts[::-1]).copy().astype(dtype)
    return ts + steps_offset if spacing == "leading" else ts


def _sigma_to_t(sigma, log_sigmas):
    """the fractional training timestep at which the table of `log_sigmas`, interpolated, gives log `sigma`"""
    log_sigma = np.log(np.maximum(sigma, 1e-10))
    dists = log_sigma - log_sigmas[:, np.newaxis]
    low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
    high_idx = low_idx + 1
    low, high = log_sigmas[low_idx], log_sigmas[high_idx]
    w = np.clip((low - log_sigma) / (low - high), 0, 1)
    return ((1 - w) * low_idx + w * high_idx).reshape(np.shape(sigma))


def _karras_schedule(lo, hi, n: int, log_sigmas, rounded: bool, rho: float = 7.0):
    """-> (sigmas, timesteps): the noise levels of Karras et al. (2022) from `hi` down to `lo`, float64, and the training timestep of
    each. The end points' roots are taken in the arithmetic `lo` and `hi` arrive in -- float32 numpy scalars (DPM-Solver), float64
    numpy scalars (Euler) or Python floats (Heun, DPM2, UniPC) -- which is why the callers convert them, not this function.
    `rounded`: DPM2, DPM-Solver and UniPC round the timesteps, Euler and Heun keep the fractions."""
    lo, hi = lo ** (1 / rho), hi ** (1 / rho)
    sigmas = (hi + np.linspace(0, 1, n) * (lo - hi)) ** rho
    ts = np.array([_sigma_to_t(s, log_sigmas) for s in sigmas])
    return sigmas, ts.round() if rounded else ts


def _check_prediction_type(pt: str, accepted=("epsilon", "v_prediction")):
    """the sigma-schedule classes' check: "sample" outside `accepted` is unimplemented, anything else outside it is refused"""
    if pt == "sample" and pt not in accepted:
        raise NotImplementedError("prediction_type not implemented yet: sample")
    if pt not in accepted:
        raise ValueError(f"prediction_type given as {pt} must be one of `epsilon`, or `v_prediction`")


def _sigma_x0(pt: str, sample, model_output, sigma):
    """x0 of a sigma-space step (after ``_check_prediction_type``: what is neither epsilon nor v is a sample prediction). `sigma`: a
    float, or a 0-dim tensor, in whose dtype the scalar expressions are then rounded."""
    if pt == "epsilon":
        return sample - sigma * model_output
    if pt == "v_prediction":
        return model_output * (-sigma / (sigma ** 2 + 1) ** 0.5) + (sample / (sigma ** 2 + 1))
    return model_output


def _sigma_derivative_pq(pt: str, sigma) -> Tuple[float, float]:
    """(p, q) with (x - x0) / sigma = p*x + q*model_output for the x0 of ``_sigma_x0``, in float64:
      epsilon       x0 = x - s e                                 ->  e
      v_prediction  x0 = x / (s^2 + 1) - v s / sqrt(s^2 + 1)     ->  x s / (s^2 + 1) + v / sqrt(s^2 + 1)
      sample        x0 = e                                       ->  (x - e) / s
    sigma = 0 gives inf or nan, which the caller refuses."""
    with np.errstate(all="ignore"):
        s_in = np.float64(sigma)
        if pt == "epsilon":
            return 0.0, 1.0
        if pt == "v_prediction":
            return float(s_in / (s_in ** 2 + 1)), float(1.0 / (s_in ** 2 + 1) ** 0.5)
        return float(1.0 / s_in), float(-1.0 / s_in)


def _euler_ab(pt: str, s: float, dt: float) -> Tuple[float, float]:
    """(a, b) with x + dt * (x - x0) / s = a*x + b*model_output for epsilon or v prediction: the row of Euler (which writes it out
    in ``step_coefficients``, where a call would show in the row's host time) and Euler a. Not
    ``1 + dt * p, dt * q`` of ``_sigma_derivative_pq``: here dt * s is formed before the division, which rounds differently from
    dt * (s / (s^2 + 1)) in the last bit, and the rows both classes were recorded with hold that bit."""
    if pt == "v_prediction":
        return 1.0 + dt * s / (s ** 2 + 1), dt / (s ** 2 + 1) ** 0.5
    return 1.0, dt


def _sigma_to_alpha_sigma_t(sigma):
    alpha_t = 1 / ((sigma ** 2 + 1) ** 0.5)
    return alpha_t, sigma * alpha_t


def _check_alpha_prediction_type(pt: str, who: str):
    if pt not in ("epsilon", "sample", "v_prediction"):
        raise ValueError(f"prediction_type given as {pt} must be one of `epsilon`, `sample`, or `v_prediction` for the {who}.")


def _alpha_convert(pt: str, to_x0: bool, a: float, s: float, sample, model_output):
    """model output -> x0 prediction (`to_x0`: dpmsolver++, UniPC's predict_x0) or epsilon prediction, at alpha_t = a, sigma_t = s"""
    if to_x0:
        return (sample - s * model_output) / a if pt == "epsilon" else model_output if pt == "sample" else a * sample - s * model_output
    return model_output if pt == "epsilon" else (sample - a * model_output) / s if pt == "sample" else a * model_output + s * sample


def _alpha_convert_pq(pt: str, to_x0: bool, a: float, s: float) -> Tuple[float, float]:
    """(p, q) with ``_alpha_convert`` = p * sample + q * model_output"""
    if to_x0:
        return (1.0 / a, -s / a) if pt == "epsilon" else (0.0, 1.0) if pt == "sample" else (a, -s)
    return (0.0, 1.0) if pt == "epsilon" else (1.0 / s, -a / s) if pt == "sample" else (s, a)


def _multistep_schedule(alphas_cumprod, c, n: int, karras_ends_as_float: bool):
    """-> (sigmas, timesteps) of the alpha-space multistep classes (DPM-Solver, UniPC): n + 1 spacing points with the last dropped,
    the sigmas interpolated at them or a Karras ramp over the whole training table, and one closing sigma -- the training table's
    smallest, or on a Karras schedule the ramp's last once more. `karras_ends_as_float`: UniPC takes the ramp's end points through
    ``.item()`` (float64 roots), DPM-Solver as the table's float32 numpy scalars (float32 roots)."""
    ts = _spaced_timesteps(c.timestep_spacing, c.num_train_timesteps, n, c.steps_offset, dtype=np.int64, drop_last=True)
    sigmas = np.array(_sigmas_of(alphas_cumprod))
    if c.use_karras_sigmas:
        lo, hi = (sigmas[0].item(), sigmas[-1].item()) if karras_ends_as_float else (sigmas[0], sigmas[-1])
        s, ts = _karras_schedule(lo, hi, n, np.log(sigmas), rounded=True)
        sigmas = np.concatenate([s, s[-1:]]).astype(np.float32)
    else:
        sigmas = np.interp(ts, np.arange(0, len(sigmas)), sigmas)
        sigmas = np.concatenate([sigmas, [_sigmas_of(alphas_cumprod[0])]]).astype(np.float32)
    return sigmas, ts.astype(np.int64)


def _init_multistep_index(self, timestep):
    """``_init_step_index`` of DPM-Solver and UniPC"""
    c = np.nonzero(self.timesteps == int(timestep))[0]
    # "the sigma index that is taken for the **very** first `step` is always the second index": an img2img start on a
    # duplicated timestep must not skip a sigma. A timestep that is not in the schedule: the last index
    self._step_index = len(self.timesteps) - 1 if len(c) == 0 else int(c[1] if len(c) > 1 else c[0])


def _alpha_sigma_floats(sigma) -> Tuple[float, float]:
    a, s = _sigma_to_alpha_sigma_t(sigma)
    return float(a), float(s)


def _out(prev, return_dict, **extra):
    if not return_dict:
        return (prev,)
    return SimpleNamespace(prev_sample=prev, **extra)


def _coefficient_walk(*fields):
    """-> the ``coefficient_walk`` method of a scheduler whose ``*_coefficients`` advance the step state in `fields` as ``step`` does:
    ``with scheduler.coefficient_walk():`` puts that state back on exit, so a loop can tabulate its rows ahead of its steps. Lists are
    copied one level deep (the walk replaces their entries, never mutates one); nothing else of the scheduler is copied."""

    @contextmanager
    def coefficient_walk(self):
        saved = {k: (list(v) if isinstance(v, list) else v) for k, v in ((k, getattr(self, k)) for k in fields)}
        try:
            yield
        finally:
            for k, v in saved.items():
                setattr(self, k, v)

    return coefficient_walk


# what a ``*_coefficients`` walk leaves where ``step`` would leave a tensor: UniPCMultistepScheduler.last_sample ("a predictor has
# run"), the entries of PNDMScheduler.ets and its cur_sample
_WALKED = object()

_NO_STEPS = "Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler"


class _Schedule:
    """What every class with a beta schedule shares; on its own, the base of the alpha-space classes (DDIM, PNDM, DPM-Solver,
    UniPC, LCM). ``__init__`` of a class:  ``self._capture(locals())`` , its refusals, ``self._build()`` ."""
    order = 1
    _train_arithmetic = "numpy"       # see _train_table
    _names_class_in_refusal = False   # the beta-schedule refusal of Heun and DPM2 names the class, as their reference's does

    def _capture(self, arguments):
        self.config = SimpleNamespace(**{k: v for k, v in arguments.items() if k != "self"})

    def _build(self):
        """the training table, the state of a scheduler that no ``set_timesteps`` has run on ("all values"), the class's ``_reset``"""
        c = self.config
        if getattr(c, "trained_betas", None) is not None:
            raise NotImplementedError(f"{self.__class__.__name__}(mi355x): trained_betas is not implemented")
        self.alphas_cumprod, train_sigmas = _train_table(c.num_train_timesteps, c.beta_start, c.beta_end, c.beta_schedule,
                                                         self._train_arithmetic, self.__class__ if self._names_class_in_refusal else None)
        self._all_values(train_sigmas)
        self._reset()

    def _all_values(self, train_sigmas):
        """alpha space: the whole training schedule, descending (a class that needs sigmas takes them from ``alphas_cumprod`` as it
        stands when ``set_timesteps`` runs)"""
        c = self.config
        if hasattr(c, "set_alpha_to_one"):
            self.final_alpha_cumprod = np.float32(1.0) if c.set_alpha_to_one else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = np.arange(0, c.num_train_timesteps)[::-1].copy().astype(np.int64)

    def _reset(self):
        """the step state, which ``__init__`` and ``set_timesteps`` both leave like this (DDIM has none)"""

    @property
    def step_index(self):
        return vars(self).get("_step_index")   # (DDIM and PNDM keep none; no class-level default, which would slow every read of it)

    def _require_steps(self):
        if self.num_inference_steps is None:
            raise ValueError(_NO_STEPS)

    def scale_model_input(self, sample, timestep=None, *args, **kwargs):
        return sample

    def _table_index(self, timesteps):
        return timesteps

    def add_noise(self, original_samples, noise, timesteps):
        a = torch.as_tensor(self.alphas_cumprod)[self._table_index(timesteps)].to(original_samples.device)
        while a.dim() < original_samples.dim():
            a = a.unsqueeze(-1)
        return a ** 0.5 * original_samples + (1 - a) ** 0.5 * noise

    def __len__(self):
        return self.config.num_train_timesteps


class _SigmaSpace:
    """Mixin of the sigma-schedule classes, in front of ``_Schedule`` in their bases: the model sees  sample / sqrt(sigma^2 + 1) ,
    noise enters as  sigma * noise , and ``set_timesteps`` interpolates the training sigmas at fractional float32 timesteps. A class
    adds its table layout to ``set_timesteps``, its ``_reset``, its stage logic and its coefficients."""
    _spacing_hint = True               # Euler's unsupported-spacing message does not name the choices
    _float32_init_sigma = False        # Heun, DPM2: sqrt(max^2 + 1) in float32, their reference's tensor expression; Euler (a): float64
    _karras_ends_as_float = True       # Euler hands the interpolated end points to the ramp as float64 numpy scalars
    _karras_rounded = False            # DPM2 rounds the Karras timesteps
    _all_values_by_set_timesteps = False
    _index_counter = None              # Heun, DPM2: {timestep: ``step`` calls seen}; Euler and Euler a do not count

    def _all_values(self, train_sigmas):
        """Euler, Euler a: the training schedule itself; Heun, DPM2: ``set_timesteps`` over all of it, as their reference's do"""
        T = self.config.num_train_timesteps
        self._train_sigmas = train_sigmas
        if self._all_values_by_set_timesteps:
            return self.set_timesteps(T)
        self.sigmas = np.concatenate([train_sigmas[::-1], [0.0]]).astype(np.float32)
        self.timesteps = np.linspace(0, T - 1, T, dtype=float)[::-1].astype(np.float32)
        self.num_inference_steps = None

    def _reset(self):
        self._step_index = None

    @property
    def init_noise_sigma(self):
        m = self.sigmas.max()
        if self.config.timestep_spacing in ("linspace", "trailing"):
            return float(m)
        if self._float32_init_sigma:
            return float(np.sqrt(m * m + np.float32(1.0)))
        return (float(m) ** 2 + 1) ** 0.5

    def _interpolated_sigmas(self, ts, sig_all, n):
        return np.interp(ts, np.arange(0, len(sig_all)), sig_all)

    def _spaced_sigmas(self, n: int, T: Optional[int] = None):
        """the part of ``set_timesteps`` every sigma-schedule class shares -> (the n sigmas and a closing 0.0, the n timesteps), float32"""
        c = self.config
        self.num_inference_steps = n
        ts = _spaced_timesteps(c.timestep_spacing, T or c.num_train_timesteps, n, c.steps_offset, dtype=np.float32,
                               round_linspace=False, hint=self._spacing_hint)
        sig_all = np.array(self._train_sigmas)
        sig = self._interpolated_sigmas(ts, sig_all, n)
        if getattr(c, "use_karras_sigmas", False):
            lo, hi = (sig[-1].item(), sig[0].item()) if self._karras_ends_as_float else (sig[-1], sig[0])
            sig, ts = _karras_schedule(lo, hi, n, np.log(sig_all), self._karras_rounded)
        return np.concatenate([sig, [0.0]]).astype(np.float32), ts.astype(np.float32)

    def set_timesteps(self, num_inference_steps: int):
        self.sigmas, self.timesteps = self._spaced_sigmas(num_inference_steps)
        self._reset()

    def _init_step_index(self, timestep):
        t = float(timestep)
        idx = np.nonzero(self.timesteps == np.float32(t))[0]
        # "the sigma index that is taken for the **very** first step is always the second index" (duplicates)
        self._step_index = int(idx[1] if len(idx) > 1 else idx[0])

    def index_for_timestep(self, timestep, schedule_timesteps=None):
        """The index ``add_noise`` takes a timestep's sigma from. A class that counts its ``step`` calls (Heun, DPM2, whose timesteps
        repeat): before any step the second of two matching indices (the only one if single), afterwards the one the counter of
        ``step`` calls at this timestep points to. Euler and Euler a: the first match."""
        ts = self.timesteps if schedule_timesteps is None else schedule_timesteps
        t = float(timestep)
        idx = np.nonzero(np.asarray(ts) == np.float32(t))[0]
        if self._index_counter is None:
            pos = 0
        elif len(self._index_counter) == 0:
            pos = 1 if len(idx) > 1 else 0
        else:
            pos = self._index_counter.setdefault(t, 0)
        return int(idx[pos])

    def _count_step(self, timestep):
        t = float(timestep)
        self._index_counter[t] = self._index_counter.get(t, 0) + 1

    def scale_model_input(self, sample, timestep):
        """(Heun and DPM2 divide by a 0-dim tensor instead of a float, DPM2 at its own sigma: their own)"""
        if self._step_index is None:
            self._init_step_index(timestep)
        return sample / ((float(self.sigmas[self._step_index]) ** 2 + 1) ** 0.5)

    def model_input_scale(self, timestep) -> float:
        if self._step_index is None:
            self._init_step_index(timestep)
        return 1.0 / ((float(self.sigmas[self._step_index]) ** 2 + 1) ** 0.5)

    def add_noise(self, original_samples, noise, timesteps):   # (sigma space; _Schedule's is the alpha-space one)
        """x + noise * sigma[``index_for_timestep`` of each timestep in the current schedule]"""
        ts = np.atleast_1d(np.asarray(timesteps.detach().cpu() if torch.is_tensor(timesteps) else timesteps, dtype=np.float32))
        idx = [self.index_for_timestep(t) for t in ts]
        sigma = torch.as_tensor(np.asarray(self.sigmas, dtype=np.float32)[idx]).to(original_samples.device,
                                                                                  original_samples.dtype)
        while sigma.dim() < original_samples.dim():
            sigma = sigma.unsqueeze(-1)
        return original_samples + noise * sigma


class DDIMScheduler(_Schedule):
    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", clip_sample: bool = True, set_alpha_to_one: bool = True,
                 steps_offset: int = 0, prediction_type: str = "epsilon", clip_sample_range: float = 1.0,
                 timestep_spacing: str = "leading"):
        self._capture(locals())
        self._build()

    def set_timesteps(self, num_inference_steps: int):
        c = self.config
        if num_inference_steps > c.num_train_timesteps:
            raise ValueError("`num_inference_steps` cannot be larger than `num_train_timesteps`")
        self.num_inference_steps = num_inference_steps
        self.timesteps = _spaced_timesteps(c.timestep_spacing, c.num_train_timesteps, num_inference_steps, c.steps_offset,
                                           dtype=np.int64, hint=False)

    def _alphas(self, timestep: int) -> Tuple[float, float]:
        prev_t = timestep - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[timestep]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        return a_t, a_prev

    def _get_variance(self, timestep, prev_timestep):
        a_t = self.alphas_cumprod[timestep]
        a_prev = self.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        return (1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)

    def step_coefficients(self, timestep) -> Tuple[float, float]:
        """(a, b) with prev = a*sample + b*model_output; epsilon or v prediction, eta = 0, no clipping."""
        c = self.config
        if c.prediction_type not in ("epsilon", "v_prediction") or c.clip_sample:
            raise NotImplementedError("linear-update form needs epsilon or v prediction without clip_sample")
        a_t, a_prev = (float(v) for v in self._alphas(int(timestep)))
        if c.prediction_type == "v_prediction":
            # step(): x0 = sqrt(a_t) x - sqrt(1 - a_t) v, eps = sqrt(a_t) v + sqrt(1 - a_t) x, prev = sqrt(a_prev) x0 + sqrt(1 - a_prev) eps
            sa, sb, pa, pb = a_t ** 0.5, (1 - a_t) ** 0.5, a_prev ** 0.5, (1 - a_prev) ** 0.5
            return pa * sa + pb * sb, pb * sa - pa * sb
        a = (a_prev / a_t) ** 0.5
        b = (1 - a_prev) ** 0.5 - (a_prev * (1 - a_t) / a_t) ** 0.5
        return a, b

    def step(self, model_output, timestep, sample, eta: float = 0.0, use_clipped_model_output: bool = False,
             generator=None, variance_noise=None, return_dict: bool = True):
        self._require_steps()
        c = self.config
        t = int(timestep)
        a_t, a_prev = (float(v) for v in self._alphas(t))
        b_t = 1.0 - a_t
        if c.prediction_type == "epsilon":
            x0 = (sample - b_t ** 0.5 * model_output) / a_t ** 0.5
            eps = model_output
        elif c.prediction_type == "sample":
            x0 = model_output
            eps = (sample - a_t ** 0.5 * x0) / b_t ** 0.5
        elif c.prediction_type == "v_prediction":
            x0 = a_t ** 0.5 * sample - b_t ** 0.5 * model_output
            eps = a_t ** 0.5 * model_output + b_t ** 0.5 * sample
        else:
            raise ValueError(f"prediction_type given as {c.prediction_type} must be one of `epsilon`, `sample`, or "
                             "`v_prediction`")
        if c.clip_sample:
            x0 = x0.clamp(-c.clip_sample_range, c.clip_sample_range)
        prev_t = t - c.num_train_timesteps // self.num_inference_steps
        std = eta * float(self._get_variance(t, prev_t)) ** 0.5
        if use_clipped_model_output:
            eps = (sample - a_t ** 0.5 * x0) / b_t ** 0.5
        prev = a_prev ** 0.5 * x0 + (1 - a_prev - std ** 2) ** 0.5 * eps
        if eta > 0:
            if variance_noise is None:
                variance_noise = torch.randn(model_output.shape, generator=generator, device=model_output.device,
                                             dtype=model_output.dtype)
            prev = prev + std * variance_noise
        return _out(prev, return_dict, pred_original_sample=x0)


class PNDMScheduler(_Schedule):
    """Pseudo numerical methods for diffusion models: Runge-Kutta warm-up (``step_prk``) + linear multistep (``step_plms``);
    Stable Diffusion uses ``skip_prk_steps=True`` (crowsonkb's PLMS, scheduling_pndm.py:216-223)."""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", skip_prk_steps: bool = False, set_alpha_to_one: bool = False,
                 prediction_type: str = "epsilon", timestep_spacing: str = "leading", steps_offset: int = 0):
        self._capture(locals())
        self.pndm_order = 4
        self.cur_sample = None
        self._build()
        self._timesteps = self.timesteps
        self.prk_timesteps = self.plms_timesteps = self.timesteps = None

    def _reset(self):
        self.ets, self.counter, self.cur_model_output = [], 0, 0

    def set_timesteps(self, num_inference_steps: int):
        c = self.config
        self.num_inference_steps = n = num_inference_steps
        self._timesteps = ts = _spaced_timesteps(c.timestep_spacing, c.num_train_timesteps, n, c.steps_offset,
                                                 dtype=np.int64)[::-1].copy()   # ascending
        if c.skip_prk_steps:
            self.prk_timesteps = np.array([], dtype=np.int64)
            self.plms_timesteps = np.concatenate([ts[:-1], ts[-2:-1], ts[-1:]])[::-1].copy()
        else:
            prk = np.array(ts[-self.pndm_order:]).repeat(2) + np.tile(np.array([0, c.num_train_timesteps // n // 2]),
                                                                        self.pndm_order)
            self.prk_timesteps = (prk[:-1].repeat(2)[1:-1])[::-1].copy()
            self.plms_timesteps = ts[:-3][::-1].copy()
        self.timesteps = np.concatenate([self.prk_timesteps, self.plms_timesteps]).astype(np.int64)
        self._reset()

    def step(self, model_output, timestep, sample, return_dict: bool = True):
        if self.counter < len(self.prk_timesteps) and not self.config.skip_prk_steps:
            return self.step_prk(model_output, timestep, sample, return_dict)
        return self.step_plms(model_output, timestep, sample, return_dict)

    def step_prk(self, model_output, timestep, sample, return_dict: bool = True):
        self._require_steps()
        n, T = self.num_inference_steps, self.config.num_train_timesteps
        timestep = int(timestep)
        prev_timestep = timestep - (0 if self.counter % 2 else T // n // 2)
        timestep = int(self.prk_timesteps[self.counter // 4 * 4])
        if self.counter % 4 == 0:
            self.cur_model_output = self.cur_model_output + 1 / 6 * model_output
            self.ets.append(model_output)
            self.cur_sample = sample
        elif (self.counter - 1) % 4 == 0 or (self.counter - 2) % 4 == 0:
            self.cur_model_output = self.cur_model_output + 1 / 3 * model_output
        else:
            model_output = self.cur_model_output + 1 / 6 * model_output
            self.cur_model_output = 0
        cur_sample = self.cur_sample if self.cur_sample is not None else sample
        prev = self._get_prev_sample(cur_sample, timestep, prev_timestep, model_output)
        self.counter += 1
        return _out(prev, return_dict)

    def step_plms(self, model_output, timestep, sample, return_dict: bool = True):
        self._require_steps()
        if not self.config.skip_prk_steps and len(self.ets) < 3:
            raise ValueError(f"{self.__class__} can only be run AFTER scheduler has been run in 'prk' mode for at least 12 "
                             "iterations")
        timestep, prev_timestep = self._plms_evaluation(timestep, model_output)
        e = self.ets
        if len(e) == 1 and self.counter == 0:
            self.cur_sample = sample
        elif len(e) == 1 and self.counter == 1:
            model_output = (model_output + e[-1]) / 2
            sample, self.cur_sample = self.cur_sample, None
        elif len(e) == 2:
            model_output = (3 * e[-1] - e[-2]) / 2
        elif len(e) == 3:
            model_output = (23 * e[-1] - 16 * e[-2] + 5 * e[-3]) / 12
        else:
            model_output = (1 / 24) * (55 * e[-1] - 59 * e[-2] + 37 * e[-3] - 9 * e[-4])
        prev = self._get_prev_sample(sample, timestep, prev_timestep, model_output)
        self.counter += 1
        return _out(prev, return_dict)

    def _plms_evaluation(self, timestep, entry):
        """-> (t, t_prev) of this evaluation of ``step_plms``, after `entry` has become the newest of ``ets``. The second evaluation
        (counter == 1) stores nothing and is made one step up: it repeats the first step with the average of both outputs."""
        step = self.config.num_train_timesteps // self.num_inference_steps
        t = int(timestep)
        if self.counter == 1:
            return t + step, t
        self.ets = self.ets[-3:] + [entry]
        return t, t - step

    def _prev_sample_scalars(self, timestep, prev_timestep) -> Tuple[float, float, float, float]:
        """(a, b, p, q) of formula (9) of the PNDM paper (scheduling_pndm.py:410-453):  prev = a*sample - b*m , where for v-prediction
        m = p*sample + q*model_output  first. Float32 numpy expressions, like the reference's tables; a_t = 0 gives inf or nan (b
        keeps the reference's sign for that: negating a NaN flips its sign bit)."""
        a_t = self.alphas_cumprod[timestep]
        a_prev = self.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        b_t, b_prev = 1 - a_t, 1 - a_prev
        p, q = (float(b_t ** 0.5), float(a_t ** 0.5)) if self.config.prediction_type == "v_prediction" else (0.0, 1.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = float((a_prev / a_t) ** 0.5)
            denom = a_t * b_prev ** 0.5 + (a_t * b_t * a_prev) ** 0.5
            b = float((a_prev - a_t) / denom)
        return a, b, p, q

    def _get_prev_sample(self, sample, timestep, prev_timestep, model_output):
        if self.config.prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"prediction_type given as {self.config.prediction_type} must be one of `epsilon` or `v_prediction`")
        a, b, p, q = self._prev_sample_scalars(timestep, prev_timestep)
        if self.config.prediction_type == "v_prediction":
            model_output = q * model_output + p * sample
        return a * sample - b * model_output

    coefficient_walk = _coefficient_walk("counter", "ets", "cur_sample", "cur_model_output")   # (plms_coefficients)

    # the exact rationals of step_plms by (counter, len(ets) after the append), newest model output first
    _PLMS_WEIGHTS = {(0, 1): (1.0, 0.0, 0.0, 0.0), (1, 1): (1 / 2, 1 / 2, 0.0, 0.0), (2, 2): (3 / 2, -1 / 2, 0.0, 0.0),
                     (3, 3): (23 / 12, -16 / 12, 5 / 12, 0.0), (4, 4): (55 / 24, -59 / 24, 37 / 24, -9 / 24)}

    def plms_coefficients(self, timestep) -> Tuple[float, ...]:
        """This model evaluation of ``step_plms`` (``skip_prk_steps=True``) as a linear map of the sample x the loop holds, the model
        output e, the stored outputs h1, h2, h3 = ``ets[-2], [-3], [-4]`` after the append (on the averaging evaluation, where nothing
        is appended, h1 = ``ets[-1]``) and the parked sample P -> (a, b, p, q, w0, w1, w2, w3, slot, park, from_park, 0.0):
            m    = w0 e + w1 h1 + w2 h2 + w3 h3          a weight of 0.0: the term is not formed
            S    = P if from_park else x                  (from_park = 1.0: the second evaluation, counter == 1; nothing is appended)
            m    = p S + q m                              v-prediction; epsilon: p = 0.0 and the line is skipped
            prev = a S + b m
        and afterwards e (unconverted) is the newest stored output unless from_park, and P = x where park = 1.0 (counter == 0).
        ``slot`` is where a ring of three planes takes e: the number of outputs stored before it, mod 3, so that h1, h2, h3 are the
        planes slot - 1, slot - 2, slot - 3 (= slot, the oldest, read before e replaces it) mod 3. The twelfth value pads the row to
        48 bytes. Advances ``counter`` and the length of ``ets`` as ``step_plms`` does, with placeholders for the tensors (and for
        ``cur_sample``). t and t_prev come from ``_plms_evaluation``, as ``step_plms``' do, so a loop that starts inside the schedule
        gets that method's own second evaluation. The schedule values are those of ``_prev_sample_scalars``, which ``step_plms`` reads
        too; the weights are the exact rationals. NotImplementedError: the Runge-Kutta warm-up (``skip_prk_steps=False``),
        a prediction type other than epsilon / v_prediction, a history that does not come from a walk started at ``counter == 0`` (its
        tensors live on the host, not in the ring), a coefficient that is not finite."""
        self._require_steps()
        cfg = self.config
        if not cfg.skip_prk_steps:
            raise NotImplementedError("the fused form is PLMS alone: the Runge-Kutta warm-up is not linear in one evaluation's state")
        if cfg.prediction_type not in ("epsilon", "v_prediction"):
            raise NotImplementedError("the fused form is for epsilon or v prediction")
        c = self.counter
        if any(e is not _WALKED for e in self.ets) or len(self.ets) != (min(c - 1, 4) if c >= 2 else c):
            raise NotImplementedError("the history of this scheduler was not built by a coefficient walk from counter == 0")
        t, t_prev = self._plms_evaluation(timestep, _WALKED)
        w = self._PLMS_WEIGHTS[(min(c, 4), len(self.ets))]
        self.cur_sample = _WALKED if c == 0 else None if c == 1 else self.cur_sample
        a, b, p, q = self._prev_sample_scalars(t, t_prev)
        self.counter += 1
        row = (a, -b, p, q) + w + (float(max(c - 1, 0) % 3) if c != 1 else 1.0, float(c == 0), float(c == 1), 0.0)
        if not all(map(isfinite, row)):
            raise NotImplementedError("a PLMS coefficient of this evaluation is not finite")
        return row


class EulerDiscreteScheduler(_SigmaSpace, _Schedule):
    _spacing_hint = False
    _karras_ends_as_float = False

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", prediction_type: str = "epsilon", interpolation_type: str = "linear",
                 use_karras_sigmas: bool = False, timestep_spacing: str = "linspace", steps_offset: int = 0):
        self._capture(locals())
        self._build()

    coefficient_walk = _coefficient_walk("_step_index")   # (step_coefficients, model_input_scale)

    def _interpolated_sigmas(self, ts, sig_all, n):
        kind = self.config.interpolation_type
        if kind == "linear":
            return super()._interpolated_sigmas(ts, sig_all, n)
        if kind == "log_linear":
            return np.exp(np.linspace(np.log(sig_all[-1]), np.log(sig_all[0]), n + 1))
        raise ValueError(f"{kind} is not implemented")

    def step_coefficients(self, timestep) -> Tuple[float, float]:
        """(a, b) with prev = a*sample + b*model_output for epsilon or v prediction, s_churn = 0; advances the index."""
        pt = self.config.prediction_type
        if pt not in ("epsilon", "v_prediction"):
            raise NotImplementedError("linear-update form is for epsilon or v prediction")
        if self._step_index is None:
            self._init_step_index(timestep)
        i = self._step_index
        s, s_next = float(self.sigmas[i]), float(self.sigmas[i + 1])
        self._step_index = i + 1
        # _euler_ab(pt, s, s_next - s), written out: a call is a tenth of this row's host time (tests/test_schedule_pieces.py holds
        # the two to the same bits)
        if pt == "v_prediction":
            return 1.0 + (s_next - s) * s / (s ** 2 + 1), (s_next - s) / (s ** 2 + 1) ** 0.5
        return 1.0, s_next - s

    def step(self, model_output, timestep, sample, s_churn: float = 0.0, s_tmin: float = 0.0,
             s_tmax: float = float("inf"), s_noise: float = 1.0, generator=None, return_dict: bool = True):
        if self._step_index is None:
            self._init_step_index(timestep)
        sigma = float(self.sigmas[self._step_index])
        gamma = min(s_churn / (len(self.sigmas) - 1), 2 ** 0.5 - 1) if s_tmin <= sigma <= s_tmax else 0.0
        sigma_hat = sigma * (gamma + 1)
        if gamma > 0:
            noise = torch.randn(model_output.shape, generator=generator, device=model_output.device,
                                dtype=model_output.dtype)
            sample = sample + noise * s_noise * (sigma_hat ** 2 - sigma ** 2) ** 0.5
        pt = self.config.prediction_type
        _check_prediction_type(pt, ("epsilon", "v_prediction", "sample", "original_sample"))
        # (the reference's epsilon form takes the churned sigma_hat, its v form the schedule's sigma)
        x0 = _sigma_x0(pt, sample, model_output, sigma if pt == "v_prediction" else sigma_hat)
        derivative = (sample - x0) / sigma_hat
        dt = float(self.sigmas[self._step_index + 1]) - sigma_hat
        prev = sample + derivative * dt
        self._step_index += 1
        return _out(prev, return_dict, pred_original_sample=x0)


class EulerAncestralDiscreteScheduler(_SigmaSpace, _Schedule):
    """"Euler a" (scheduling_euler_ancestral_discrete.py:130-389): an Euler step down to sigma_down and fresh noise of sigma_up back
    up, every step. epsilon and v prediction, the three spacings; ``trained_betas`` is not implemented. The step is linear in the
    sample, the model output and the noise: ``ancestral_coefficients`` returns (a, b, c) with  prev = a*sample + b*model_output +
    c*noise  for the library's ``mi355x_sd_ancestral_update``."""
    _train_arithmetic = "tensor"

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", trained_betas=None, prediction_type: str = "epsilon",
                 timestep_spacing: str = "linspace", steps_offset: int = 0):
        self._capture(locals())
        self._build()

    coefficient_walk = _coefficient_walk("_step_index")   # (ancestral_coefficients, model_input_scale)

    def _check(self, timestep):
        _check_prediction_type(self.config.prediction_type)
        self._require_steps()
        if self._step_index is None:
            self._init_step_index(timestep)

    def _ancestral_sigmas(self):
        """(sigma, sigma_up, dt) of this step in float32, the reference's own expressions (:339-347) on its float32 sigmas"""
        s, s_to = self.sigmas[self._step_index], self.sigmas[self._step_index + 1]
        s_up = np.sqrt(s_to * s_to * (s * s - s_to * s_to) / (s * s))
        s_down = np.sqrt(s_to * s_to - s_up * s_up)
        assert s_up.dtype == s_down.dtype == np.float32
        return s, s_up, s_down - s

    def ancestral_coefficients(self, timestep) -> Tuple[float, float, float]:
        """(a, b, c) with prev = a*sample + b*model_output + c*noise, composed in float64 from the float32 sigma, sigma_up and dt of
        ``step``; advances the index. c == 0.0 exactly on the last row (sigma_to = 0). A non-finite row: NotImplementedError."""
        self._check(timestep)
        s, c, dt = (float(v) for v in self._ancestral_sigmas())
        self._step_index += 1
        a, b = _euler_ab(self.config.prediction_type, s, dt)
        if not all(map(isfinite, (a, b, c))):
            raise NotImplementedError("a non-finite row has no linear-update form")
        return a, b, c

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True, *, noise=None):
        """-> prev_sample and pred_original_sample. ``noise`` (extension): this step's draw, otherwise ``torch.randn`` from
        ``generator`` -- on every step, the last included (sigma_up = 0 there), as the reference draws."""
        if isinstance(timestep, int) or (torch.is_tensor(timestep) and not timestep.is_floating_point()):
            raise ValueError("Passing integer indices (e.g. from `enumerate(timesteps)`) as timesteps to `EulerDiscreteScheduler.step()` "
                             "is not supported. Make sure to pass one of the `scheduler.timesteps` as a timestep.")
        self._check(timestep)
        s, s_up, dt = (float(v) for v in self._ancestral_sigmas())
        x0 = _sigma_x0(self.config.prediction_type, sample, model_output, s)
        derivative = (sample - x0) / s
        prev = sample + derivative * dt
        if noise is None:
            noise = torch.randn(model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
        prev = prev + noise * s_up
        self._step_index += 1
        return _out(prev, return_dict, pred_original_sample=x0)


class HeunDiscreteScheduler(_SigmaSpace, _Schedule):
    """"Heun" (scheduling_heun_discrete.py:71-480): the second-order k-diffusion sampler, two model evaluations per step. Every
    timestep but the first appears twice; the first evaluation of a pair takes an Euler step and parks the sample, the derivative and
    dt, the second averages the two derivatives and steps again from the parked sample; the last step (to sigma = 0) is a plain Euler
    step. epsilon, v_prediction and sample prediction, the three spacings, Karras sigmas, ``clip_sample``; ``trained_betas`` is not
    implemented. Both stages are linear in the current sample, the model output and the parked state: ``heun_coefficients`` returns
    (p, q, h, g, second) for the library's ``mi355x_sd_heun_update``."""
    order = 2
    _train_arithmetic = "tensor"
    _names_class_in_refusal = True
    _float32_init_sigma = True
    _all_values_by_set_timesteps = True

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "linear", trained_betas=None, prediction_type: str = "epsilon",
                 use_karras_sigmas: bool = False, clip_sample: bool = False, clip_sample_range: float = 1.0,
                 timestep_spacing: str = "linspace", steps_offset: int = 0):
        self._capture(locals())
        self._build()
        self.use_karras_sigmas = use_karras_sigmas

    @property
    def state_in_first_order(self):
        return self.dt is None

    coefficient_walk = _coefficient_walk("_step_index", "dt")   # (heun_coefficients, model_input_scale)

    def set_timesteps(self, num_inference_steps: int):
        sig, ts = self._spaced_sigmas(num_inference_steps)   # (:213-277; the Karras timesteps are not rounded, :304-327)
        # [s0, s1, s1, ..., s_{n-1}, s_{n-1}, 0] and [t0, t1, t1, ..., t_{n-1}, t_{n-1}]: 2n sigmas, 2n - 1 timesteps
        self.sigmas = np.concatenate([sig[:1], np.repeat(sig[1:-1], 2), sig[-1:]])
        self.timesteps = np.concatenate([ts[:1], np.repeat(ts[1:], 2)])
        self._reset()

    def _reset(self):
        self.prev_derivative = self.dt = self.sample = None
        self._step_index: Optional[int] = None
        self._index_counter = {}

    def _sigma(self, i, dtype):
        """sigmas[i] as a 0-dim tensor of `dtype`: the reference casts its sigma tensor to the model output's dtype (:376-377), so the
        scalar expressions of ``step`` are rounded in that dtype"""
        return torch.tensor(float(self.sigmas[i]), dtype=dtype)

    def scale_model_input(self, sample, timestep):
        if self._step_index is None:
            self._init_step_index(timestep)
        sigma = self._sigma(self._step_index, sample.dtype)
        return sample / ((sigma ** 2 + 1) ** 0.5)

    def _check(self, timestep):
        _check_prediction_type(self.config.prediction_type, ("epsilon", "v_prediction", "sample"))
        if self._step_index is None:
            self._init_step_index(timestep)

    def heun_coefficients(self, timestep) -> Tuple[float, float, float, float, float]:
        """(p, q, h, g, second): the row of the step ``step`` would take now, composed in float64 from the float32 sigmas; advances the
        index and the stage (``dt``) as ``step`` does. With d = p*sample + q*model_output,
          second == 0 (first order):  prev = sample + h*d, and the launch parks sample and d           h = dt = sigma_next - sigma
          second == 1 (Heun):         prev = parked sample + h*(g*parked d + d)                        h = dt / 2 of the parked dt, g = 1
        g weights the parked derivative: Heun's average takes 1; a midpoint method (KDPM2) would take 0 and never read it.
        ``clip_sample`` is not linear, a non-finite row has no such form: NotImplementedError."""
        self._check(timestep)
        if self.config.clip_sample:
            raise NotImplementedError("clip_sample has no linear-update form")
        i, first = self._step_index, self.dt is None
        if first:
            s, s_next = float(self.sigmas[i]), float(self.sigmas[i + 1])
            s_in, h, g, second = s, s_next - s, 0.0, 0.0
            self.dt = h
        else:
            s_in, h, g, second = float(self.sigmas[i]), float(self.dt) / 2, 1.0, 1.0
            self.dt = None
        self._step_index += 1
        p, q = _sigma_derivative_pq(self.config.prediction_type, s_in)
        if not all(map(isfinite, (p, q, h))):
            raise NotImplementedError("a non-finite row has no linear-update form")
        return p, q, h, g, second

    def step(self, model_output, timestep, sample, return_dict: bool = True):
        """(:349-455) line by line; the sigmas enter as 0-dim tensors of the model output's dtype"""
        self._check(timestep)
        self._count_step(timestep)
        i, dtype, c = self._step_index, model_output.dtype, self.config
        first = self.state_in_first_order
        if first:
            sigma, sigma_next = self._sigma(i, dtype), self._sigma(i + 1, dtype)
        else:   # 2nd order / Heun's method
            sigma, sigma_next = self._sigma(i - 1, dtype), self._sigma(i, dtype)
        sigma_hat = sigma   # gamma = 0
        x0 = _sigma_x0(c.prediction_type, sample, model_output, sigma_hat if first else sigma_next)
        if c.clip_sample:
            x0 = x0.clip(-c.clip_sample_range, c.clip_sample_range)
        if first:
            derivative = (sample - x0) / sigma_hat
            dt = sigma_next - sigma_hat
            self.prev_derivative, self.dt, self.sample = derivative, dt, sample
        else:
            derivative = (sample - x0) / sigma_next
            derivative = (self.prev_derivative + derivative) / 2
            dt, sample = self.dt, self.sample
            self.prev_derivative = self.dt = self.sample = None   # back in first-order mode
        prev = sample + derivative * dt
        self._step_index += 1
        return _out(prev, return_dict)


class KDPM2DiscreteScheduler(_SigmaSpace, _Schedule):
    """"DPM2" (scheduling_k_dpm_2_discrete.py:71-487): the second-order k-diffusion midpoint sampler, two model evaluations per step.
    The first evaluation of a step takes an Euler step to ``sigma_interpol``, the geometric mean of the step's two sigmas, and parks
    the sample; the second is made there (its timestep comes from ``_sigma_to_t``) and takes the whole step from the parked sample
    with the new derivative alone; the last step (to sigma = 0) is a plain Euler step. epsilon and v prediction, the three spacings,
    ``steps_offset``, Karras sigmas; ``trained_betas`` and ``squaredcos_cap_v2`` are not implemented, ``prediction_type="sample"`` is
    refused by ``step`` as the reference refuses it. Both stages are linear in the current sample, the model output and the parked
    sample: ``dpm2_coefficients`` returns (p, q, h, c, second) for the library's ``mi355x_sd_dpm2_update``.

    The tables are built in the reference's float32 tensor arithmetic; its ``Tensor.lerp`` is taken as ``torch.lerp``. ``step`` carries
    ``sigmas`` as 0-dim tensors of the model output's dtype, as the reference's cast does; the reference leaves its other tables
    (``sigmas_interpol``, and the ancestral class's ``sigmas_up`` / ``sigmas_down``) float32, and so does ``step`` -- but for a float64
    model output, which takes them in float64 too (the float64 loops of the tests are this project's measuring stick)."""
    order = 2
    _train_arithmetic = "tensor"
    _names_class_in_refusal = True
    _float32_init_sigma = True
    _karras_rounded = True   # (:252)
    _all_values_by_set_timesteps = True

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "linear", trained_betas=None, use_karras_sigmas: bool = False,
                 prediction_type: str = "epsilon", timestep_spacing: str = "linspace", steps_offset: int = 0):
        self._capture(locals())
        self._build()

    @property
    def state_in_first_order(self):
        return self.sample is None

    coefficient_walk = _coefficient_walk("_step_index", "sample")   # (dpm2_coefficients, model_input_scale)

    @staticmethod
    def _tables(sig):
        """the per-step tables beside the sigmas (:258-261), and which of their interpolated timesteps sit between the steps'"""
        interpol = sig.log().lerp(sig.roll(1).log(), 0.5).exp()
        interpol[-1] = 0.0
        return dict(sigmas_interpol=interpol), slice(1, -1)

    def _stage(self, i, first):
        """float32 (sigma, sigma_interpol, the sigma stage 2 steps to, sigma_up) of the evaluation at index i (:400-409)"""
        if first:
            return self.sigmas[i], self.sigmas_interpol[i + 1], None, None
        return self.sigmas[i - 1], self.sigmas_interpol[i], self.sigmas[i], None

    def set_timesteps(self, num_inference_steps: int, num_train_timesteps: Optional[int] = None):
        sig, ts = self._spaced_sigmas(num_inference_steps, num_train_timesteps)
        sig = torch.from_numpy(sig)
        # entries no evaluation reads go through log(0) and inf - inf on the way, as in the reference
        tables, between = self._tables(sig)
        for k, v in dict(tables, sigmas=sig).items():   # [v0, v1, v1, ..., vn, vn, vn]: 2n + 2 entries
            setattr(self, k, torch.cat([v[:1], v[1:].repeat_interleave(2), v[-1:]]).numpy())
        with np.errstate(all="ignore"):
            # (one call over the array: the per-element arithmetic of the reference's loop over _sigma_to_t)
            t_interpol = _sigma_to_t(tables["sigmas_interpol"].numpy(), np.log(np.array(self._train_sigmas))).astype(np.float32)
        # [t0, t'0, t1, t'1, ..., t_{n-1}]: 2n - 1 timesteps, t'k the timestep of the sigma stage 2 of step k is evaluated at
        self.timesteps = np.concatenate([ts[:1], np.stack((t_interpol[between], ts[1:]), axis=-1).reshape(-1)])
        self._reset()

    def _reset(self):
        self.sample = None
        self._step_index: Optional[int] = None
        self._index_counter = {}

    def _sigma_in(self):
        """the float32 sigma the model is evaluated at now: ``sigmas`` in stage 1, ``sigmas_interpol`` in stage 2 (:200-204)"""
        first = self.state_in_first_order
        return self._stage(self._step_index, first)[0 if first else 1]

    def scale_model_input(self, sample, timestep):
        if self._step_index is None:
            self._init_step_index(timestep)
        sigma = torch.tensor(float(self._sigma_in()), dtype=torch.promote_types(torch.float32, sample.dtype))
        return sample / ((sigma ** 2 + 1) ** 0.5)

    def model_input_scale(self, timestep) -> float:
        if self._step_index is None:
            self._init_step_index(timestep)
        return 1.0 / ((float(self._sigma_in()) ** 2 + 1) ** 0.5)

    def dpm2_coefficients(self, timestep) -> Tuple[float, float, float, float, float]:
        """(p, q, h, c, second): the row of the evaluation ``step`` would take now, composed in float64 from the float32 schedule
        values ``step`` uses; advances the index and the stage as ``step`` does. With d = p*sample + q*model_output, the derivative
        at the sigma the model was evaluated at,
          second == 0:  prev = sample + h*d, and the launch parks sample             h = sigma_interpol - sigma
          second == 1:  prev = parked sample + h*d [+ c*noise]                       h = sigma_next - sigma (DPM2), c = 0.0 exactly;
                                                                                     h = sigma_down - sigma, c = sigma_up (DPM2 a)
        A non-finite row has no such form: NotImplementedError."""
        if self._step_index is None:
            self._init_step_index(timestep)
        _check_prediction_type(self.config.prediction_type)
        i, first = self._step_index, self.state_in_first_order
        s, s_interpol, s_to, s_up = (None if v is None else float(v) for v in self._stage(i, first))
        if first:
            s_in, h, c, second = s, s_interpol - s, 0.0, 0.0
            self.sample = _WALKED
        else:
            s_in, h, c, second = s_interpol, s_to - s, 0.0 if s_up is None else s_up, 1.0
            self.sample = None
        self._step_index += 1
        p, q = _sigma_derivative_pq(self.config.prediction_type, s_in)
        if not all(map(isfinite, (p, q, h, c))):
            raise NotImplementedError("a non-finite row has no linear-update form")
        return p, q, h, c, second

    def _begin(self, timestep):
        if self._step_index is None:
            self._init_step_index(timestep)
        self._count_step(timestep)

    def _advance(self, model_output, sample, noise, return_dict):
        """(:411-462, ancestral :425-478) line by line from the prediction-type branch on"""
        i, dtype, first = self._step_index, model_output.dtype, self.state_in_first_order
        other = torch.promote_types(torch.float32, dtype)   # (the tables beside ``sigmas`` stay float32 in the reference)
        s, s_interpol, s_to, s_up = self._stage(i, first)
        sigma_hat = torch.tensor(float(s), dtype=dtype)   # gamma = 0
        sigma_interpol = torch.tensor(float(s_interpol), dtype=other)
        _check_prediction_type(self.config.prediction_type)
        x0 = _sigma_x0(self.config.prediction_type, sample, model_output, sigma_hat if first else sigma_interpol)
        if first:
            derivative = (sample - x0) / sigma_hat
            dt = sigma_interpol - sigma_hat
            self.sample = sample   # store for 2nd order step
            prev = sample + derivative * dt
        else:   # DPM-Solver-2
            derivative = (sample - x0) / sigma_interpol
            dt = torch.tensor(float(s_to), dtype=other) - sigma_hat
            sample, self.sample = self.sample, None
            prev = sample + derivative * dt
            if s_up is not None:
                prev = prev + noise * torch.tensor(float(s_up), dtype=other)
        self._step_index += 1
        return _out(prev, return_dict)

    def step(self, model_output, timestep, sample, return_dict: bool = True):
        self._begin(timestep)
        return self._advance(model_output, sample, None, return_dict)


class KDPM2AncestralDiscreteScheduler(KDPM2DiscreteScheduler):
    """"DPM2 a" (scheduling_k_dpm_2_ancestral_discrete.py:72-504): KDPM2DiscreteScheduler whose steps end at ``sigma_down`` and add
    fresh noise of ``sigma_up`` back, as Euler a's do. The midpoint lies between sigma and sigma_down; the noise enters in the second
    evaluation of a step only, but ``step`` draws a plane at EVERY evaluation, as the reference does, so one seed leaves the generator
    in the same state whichever path draws. ``dpm2_coefficients`` returns c = sigma_up on the second-stage rows."""

    @staticmethod
    def _tables(sig):
        """(:259-268)"""
        sig_next = sig.roll(-1)
        sig_next[-1] = 0.0
        up = (sig_next ** 2 * (sig ** 2 - sig_next ** 2) / sig ** 2) ** 0.5
        down = (sig_next ** 2 - up ** 2) ** 0.5
        down[-1] = 0.0
        interpol = sig.log().lerp(down.log(), 0.5).exp()
        interpol[-2:] = 0.0
        return dict(sigmas_interpol=interpol, sigmas_up=up, sigmas_down=down), slice(None, -2)

    def _stage(self, i, first):
        """(:413-423)"""
        if first:
            return self.sigmas[i], self.sigmas_interpol[i], None, None
        return self.sigmas[i - 1], self.sigmas_interpol[i - 1], self.sigmas_down[i - 1], self.sigmas_up[i - 1]

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True, *, noise=None):
        """``noise`` (extension): this evaluation's draw, otherwise ``torch.randn`` from ``generator`` -- at every evaluation, the
        first-order ones included, where it is not used"""
        self._begin(timestep)
        if noise is None:
            noise = torch.randn(model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
        return self._advance(model_output, sample, noise, return_dict)


class DPMSolverMultistepScheduler(_Schedule):
    """The fast multistep solver most SD pipelines switch to (20-25 steps; the reference's DiT example uses it). Implemented:
    ``algorithm_type`` "dpmsolver++" / "dpmsolver", ``solver_order`` 1-2, "midpoint" / "heun", epsilon / v_prediction / sample,
    ``lower_order_final``, ``euler_at_final``, Karras sigmas. Not implemented (NotImplementedError): the SDE variants,
    third order, thresholding, ``use_lu_lambdas``, a finite ``lambda_min_clipped``."""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", solver_order: int = 2, prediction_type: str = "epsilon",
                 thresholding: bool = False, dynamic_thresholding_ratio: float = 0.995, sample_max_value: float = 1.0,
                 algorithm_type: str = "dpmsolver++", solver_type: str = "midpoint", lower_order_final: bool = True,
                 euler_at_final: bool = False, use_karras_sigmas: bool = False, use_lu_lambdas: bool = False,
                 lambda_min_clipped: float = -float("inf"), variance_type: Optional[str] = None,
                 timestep_spacing: str = "linspace", steps_offset: int = 0):
        self._capture(locals())
        if algorithm_type not in ("dpmsolver", "dpmsolver++"):
            raise NotImplementedError(f"{algorithm_type} is not implemented for {self.__class__}")
        if solver_type not in ("midpoint", "heun"):
            raise NotImplementedError(f"{solver_type} is not implemented for {self.__class__}")
        if solver_order not in (1, 2) or thresholding or use_lu_lambdas or lambda_min_clipped != -float("inf") or variance_type:
            raise NotImplementedError("DPMSolverMultistepScheduler(mi355x): solver_order 3, thresholding, use_lu_lambdas, "
                                      "lambda_min_clipped and learned variance are not implemented")
        self._build()

    def _reset(self):
        self.model_outputs = [None] * self.config.solver_order
        self.lower_order_nums = 0
        self._step_index = None

    coefficient_walk = _coefficient_walk("_step_index", "lower_order_nums", "model_outputs")   # (multistep_coefficients)

    def set_timesteps(self, num_inference_steps: int):
        self.sigmas, self.timesteps = _multistep_schedule(self.alphas_cumprod, self.config, num_inference_steps,
                                                          karras_ends_as_float=False)
        self.num_inference_steps = len(self.timesteps)
        self._reset()

    def convert_model_output(self, model_output, sample):
        """model output -> x0 prediction (dpmsolver++) or epsilon prediction (dpmsolver), :407-506"""
        c = self.config
        a, s = _alpha_sigma_floats(self.sigmas[self._step_index])
        _check_alpha_prediction_type(c.prediction_type, "DPMSolverMultistepScheduler")
        return _alpha_convert(c.prediction_type, c.algorithm_type == "dpmsolver++", a, s, sample, model_output)

    _init_step_index = _init_multistep_index
    _sigma_to_alpha_sigma_t = staticmethod(_sigma_to_alpha_sigma_t)

    def _update_scalars(self):
        """The scalars of the update from sigma index ``_step_index`` to the next -> (A, b, c, plus, r_inv), each a float of a float32
        numpy expression (alpha_t, sigma_t, lambda, h and the coefficients, as the reference's float32 tensors give them):
            prev = A x - b m0                                  first order (:508-575), c = plus = r_inv = None
            prev = A x - b m0 -/+ c (r_inv (m0 - m1))          second-order multistep (:577-698), r_inv = 1 / r0; + where `plus`
        ``step`` and ``multistep_coefficients`` both read this and nothing else of the schedule. b and c come with the sign the
        reference's expressions give them, and `plus` apart, not folded in: a Karras schedule repeats its last sigma, h = 0 gives
        r_inv = 0 like the reference and heun's 0 / 0 a NaN c, and negating a NaN flips the sign bit ``step`` then returns."""
        c, n, i = self.config, len(self.timesteps), self._step_index
        lower_order_final = i == n - 1 and (c.euler_at_final or (c.lower_order_final and n < 15))
        at, st = _sigma_to_alpha_sigma_t(self.sigmas[i + 1])
        a0, s0 = _sigma_to_alpha_sigma_t(self.sigmas[i])
        lt, l0 = np.log(at) - np.log(st), np.log(a0) - np.log(s0)
        h = lt - l0
        pp, f = c.algorithm_type == "dpmsolver++", float
        A, b = (f(st / s0), f(at * (np.exp(-h) - 1.0))) if pp else (f(at / a0), f(st * (np.exp(h) - 1.0)))
        if c.solver_order == 1 or self.lower_order_nums < 1 or lower_order_final:
            return A, b, None, None, None
        # (with solver_order <= 2 the second-order branch is taken whenever history exists)
        a1, s1 = _sigma_to_alpha_sigma_t(self.sigmas[i - 1])
        h_0 = l0 - (np.log(a1) - np.log(s1))
        with np.errstate(divide="ignore", invalid="ignore"):
            r_inv = f(1.0 / (h_0 / h))
            if c.solver_type == "midpoint":
                return A, b, f(0.5 * at * (np.exp(-h) - 1.0)) if pp else f(0.5 * st * (np.exp(h) - 1.0)), False, r_inv
            return A, b, f(at * ((np.exp(-h) - 1.0) / h + 1.0)) if pp else f(st * ((np.exp(h) - 1.0) / h - 1.0)), pp, r_inv

    def _advance(self):
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True):
        self._require_steps()
        if self._step_index is None:
            self._init_step_index(timestep)
        m = self.convert_model_output(model_output, sample)
        self.model_outputs = self.model_outputs[1:] + [m]
        A, b, c, plus, r_inv = self._update_scalars()
        prev = A * sample - b * m
        if c is not None:
            d1 = r_inv * (m - self.model_outputs[-2])
            prev = prev + c * d1 if plus else prev - c * d1
        self._advance()
        return _out(prev, return_dict)

    def multistep_coefficients(self, timestep) -> Tuple[float, float, float, float, float]:
        """(p, q, A, B, D) of this step's update as a linear map of the sample x, the model output e and the previous step's
        converted output m1:  m0 = p x + q e  (``convert_model_output``),  prev = A x + B m0 + D (m0 - m1) ; D = 0 on a first-order
        step. Advances ``_step_index`` and ``lower_order_nums`` as ``step`` does. The schedule values are ``_update_scalars``' and the
        alpha_t, sigma_t of ``convert_model_output``, the very numbers ``step`` reads; the five are composed from them in float64.
        NotImplementedError when one of them is not finite (heun's 0 / 0 on a Karras schedule's repeated last sigma, where ``step``
        itself yields NaN)."""
        self._require_steps()
        if self._step_index is None:
            self._init_step_index(timestep)
        cfg = self.config
        if cfg.prediction_type not in ("epsilon", "sample", "v_prediction"):
            raise NotImplementedError(f"prediction_type {cfg.prediction_type}")
        a, s = _alpha_sigma_floats(self.sigmas[self._step_index])
        p, q = _alpha_convert_pq(cfg.prediction_type, cfg.algorithm_type == "dpmsolver++", a, s)
        A, b, c, plus, r_inv = self._update_scalars()
        B, D = -b, 0.0 if c is None else (c if plus else -c) * r_inv
        self._advance()
        if not all(map(isfinite, (p, q, A, B, D))):
            raise NotImplementedError("a multistep coefficient of this step is not finite")
        return p, q, A, B, D


class UniPCMultistepScheduler(_Schedule):
    """UniPC (scheduling_unipc_multistep.py:31-846): a B(h) predictor of order 1-3 (``multistep_uni_p_bh_update``) whose output the
    next step corrects with the model output it was evaluated at (``multistep_uni_c_bh_update``), usable at 8-15 steps. Implemented:
    ``solver_order`` 1-3, "bh1" / "bh2" ("midpoint" / "heun" / "logrho" become "bh2"), ``predict_x0``, epsilon / sample / v_prediction,
    ``lower_order_final``, ``disable_corrector``, Karras sigmas, the three spacings. Not implemented (NotImplementedError):
    thresholding, ``solver_p``, ``trained_betas``.
    Both halves are linear in the tensors with scalars of the schedule alone: ``unipc_coefficients`` returns them as one row for the
    library's ``mi355x_sd_unipc_update``."""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", trained_betas=None, solver_order: int = 2, prediction_type: str = "epsilon",
                 thresholding: bool = False, dynamic_thresholding_ratio: float = 0.995, sample_max_value: float = 1.0,
                 predict_x0: bool = True, solver_type: str = "bh2", lower_order_final: bool = True, disable_corrector=(),
                 solver_p=None, use_karras_sigmas: bool = False, timestep_spacing: str = "linspace", steps_offset: int = 0):
        disable_corrector = list(disable_corrector)
        if solver_type not in ("bh1", "bh2"):
            if solver_type not in ("midpoint", "heun", "logrho"):
                raise NotImplementedError(f"{solver_type} is not implemented for {self.__class__}")
            solver_type = "bh2"
        self._capture(locals())
        if thresholding or solver_p is not None or trained_betas is not None or solver_order not in (1, 2, 3):
            raise NotImplementedError("UniPCMultistepScheduler(mi355x): thresholding, solver_p, trained_betas and solver_order "
                                      "outside 1-3 are not implemented")
        self.predict_x0, self.disable_corrector, self.solver_p = predict_x0, disable_corrector, None
        self.timestep_list = [None] * solver_order
        self.this_order = None
        self._build()

    def _reset(self):
        self.model_outputs = [None] * self.config.solver_order
        self.lower_order_nums = 0
        self.last_sample = None
        self._step_index = None

    coefficient_walk = _coefficient_walk("_step_index", "lower_order_nums", "model_outputs", "timestep_list", "last_sample",
                                         "this_order")   # (unipc_coefficients)

    def set_timesteps(self, num_inference_steps: int):
        self.sigmas, self.timesteps = _multistep_schedule(self.alphas_cumprod, self.config, num_inference_steps,
                                                          karras_ends_as_float=True)
        self.num_inference_steps = len(self.timesteps)
        self._reset()

    _init_step_index = _init_multistep_index
    _sigma_to_alpha_sigma_t = staticmethod(_sigma_to_alpha_sigma_t)

    def _alpha_sigma(self) -> Tuple[float, float]:
        _check_alpha_prediction_type(self.config.prediction_type, "UniPCMultistepScheduler")
        return _alpha_sigma_floats(self.sigmas[self._step_index])

    def convert_model_output(self, model_output, *args, sample=None, **kwargs):
        """model output -> x0 prediction (predict_x0) or epsilon prediction, :368-436"""
        if sample is None:
            if len(args) < 2:
                raise ValueError("missing `sample` as a required keyward argument")
            sample = args[1]
        return _alpha_convert(self.config.prediction_type, self.predict_x0, *self._alpha_sigma(), sample, model_output)

    def _bh_scalars(self, i_t: int, i_s0: int, older, order: int, corrector: bool):
        """The float32 scalars of one B(h) update from sigma index i_s0 to i_t (:490-546 / :625-683), ``older`` the sigma indices of
        the history entries behind m0 -> (A, B, G, rks, rhos):  x_t = A x - B m0 - G (sum_k rhos[k] (m_k - m0) / rks[k] [+ rhos[-1]
        (m_t - m0)]). The predictor solves for ``order - 1`` rhos (0.5 at order 2), the corrector for ``order`` (0.5 at order 1), in
        float32 like the reference's linalg.solve. A repeated sigma (h = 0) gives what the reference gets: inf and nan."""
        f32 = np.float32
        with np.errstate(divide="ignore", invalid="ignore"):
            at, st = self._sigma_to_alpha_sigma_t(self.sigmas[i_t])
            a0, s0 = self._sigma_to_alpha_sigma_t(self.sigmas[i_s0])
            l0 = np.log(a0) - np.log(s0)
            h = (np.log(at) - np.log(st)) - l0
            rks = []
            for si in older:
                ai, s_i = self._sigma_to_alpha_sigma_t(self.sigmas[si])
                rks.append(((np.log(ai) - np.log(s_i)) - l0) / h)
            rk_all = np.array(rks + [1.0], dtype=np.float32)
            hh = -h if self.predict_x0 else h
            h_phi_1 = np.expm1(hh)
            h_phi_k = h_phi_1 / hh - f32(1)
            B_h = hh if self.config.solver_type == "bh1" else np.expm1(hh)
            R, b, factorial_i = [], [], 1
            for i in range(1, order + 1):
                R.append(rk_all ** (i - 1))
                b.append(h_phi_k * f32(factorial_i) / B_h)
                factorial_i *= i + 1
                h_phi_k = h_phi_k / hh - f32(1 / factorial_i)
            R, b = np.stack(R).astype(np.float32), np.array(b, dtype=np.float32)
            if corrector:
                rhos = np.array([0.5], dtype=np.float32) if order == 1 else self._solve(R, b)
            else:
                rhos = np.zeros(0, np.float32) if order == 1 else np.array([0.5], dtype=np.float32) if order == 2 else \
                    self._solve(R[:-1, :-1], b[:-1])
            if self.predict_x0:
                return st / s0, at * h_phi_1, at * B_h, rks, rhos
            return at / a0, st * h_phi_1, st * B_h, rks, rhos

    @staticmethod
    def _solve(R, b):
        try:
            return np.linalg.solve(R, b).astype(np.float32)   # float32 in, LAPACK's single-precision solve
        except np.linalg.LinAlgError:
            return np.full(len(b), np.nan, dtype=np.float32)

    def _bh_update(self, x, m0, older_outputs, model_t, scalars):
        A, B, G, rks, rhos = scalars
        f = float
        with np.errstate(divide="ignore", invalid="ignore"):
            res = 0
            for k, (mk, rk) in enumerate(zip(older_outputs, rks)):
                res = res + f(rhos[k]) * ((mk - m0) / f(rk))
            if model_t is not None:
                res = res + f(rhos[-1]) * (model_t - m0)
        return f(A) * x - f(B) * m0 - f(G) * res

    def multistep_uni_p_bh_update(self, model_output, *args, sample=None, order=None, **kwargs):
        """UniP, the B(h) predictor (:438-565): ``sample`` at sigma index step_index -> step_index + 1"""
        if sample is None or order is None:
            raise ValueError(" missing `sample` / `order` as a required keyward argument")
        i = self._step_index
        sc = self._bh_scalars(i + 1, i, [i - k for k in range(1, order)], order, corrector=False)
        return self._bh_update(sample, self.model_outputs[-1], [self.model_outputs[-(k + 1)] for k in range(1, order)], None, sc)

    def multistep_uni_c_bh_update(self, this_model_output, *args, last_sample=None, this_sample=None, order=None, **kwargs):
        """UniC, the B(h) corrector (:567-701): ``last_sample`` at sigma index step_index - 1 -> step_index, with the model output
        converted at ``this_sample``"""
        if last_sample is None or this_sample is None or order is None:
            raise ValueError(" missing `last_sample` / `this_sample` / `order` as a required keyward argument")
        i = self._step_index
        sc = self._bh_scalars(i, i - 1, [i - (k + 1) for k in range(1, order)], order, corrector=True)
        return self._bh_update(last_sample, self.model_outputs[-1], [self.model_outputs[-(k + 1)] for k in range(1, order)],
                               this_model_output, sc)

    def _use_corrector(self):
        return self._step_index > 0 and self._step_index - 1 not in self.disable_corrector and self.last_sample is not None

    def _next_order(self):
        c = self.config
        this_order = min(c.solver_order, len(self.timesteps) - self._step_index) if c.lower_order_final else c.solver_order
        return min(this_order, self.lower_order_nums + 1)   # warm-up of the multistep history

    def step(self, model_output, timestep, sample, return_dict: bool = True):
        self._require_steps()
        if self._step_index is None:
            self._init_step_index(timestep)
        m = self.convert_model_output(model_output, sample=sample)   # at the UNCORRECTED sample, as the reference does
        if self._use_corrector():
            sample = self.multistep_uni_c_bh_update(this_model_output=m, last_sample=self.last_sample, this_sample=sample,
                                                    order=self.this_order)
        self.model_outputs = self.model_outputs[1:] + [m]
        self.timestep_list = self.timestep_list[1:] + [timestep]
        self.this_order = self._next_order()
        self.last_sample = sample
        prev = self.multistep_uni_p_bh_update(model_output=model_output, sample=sample, order=self.this_order)
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1
        return _out(prev, return_dict)

    def unipc_coefficients(self, timestep) -> Tuple[float, ...]:
        """This step as a linear map of the sample x the loop holds, the model output e, ``last_sample`` L and the history h1, h2, h3 =
        ``model_outputs[-1], [-2], [-3]`` before the step's shift -> (p, q, Ac, Bc, C2, C3, Ct, Ap, Bp, D1, D2, corr):
            m_t  = p x + q e
            x_c  = Ac L + Bc h1 + C2 (h2 - h1) + C3 (h3 - h1) + Ct (m_t - h1)      corr == 1.0; corr == 0.0: x_c = x
            prev = Ap x_c + Bp m_t + D1 (h1 - m_t) + D2 (h2 - m_t)
        and afterwards last_sample = x_c, model_outputs = [.., h2, h1, m_t]. A term the step's order does not form has the
        coefficient 0.0. Advances ``_step_index``, ``lower_order_nums``, ``this_order`` and marks ``last_sample`` as ``step`` does.
        Every schedule value is the float32 numpy expression of ``step``; the row is composed from them in float64.
        NotImplementedError when a coefficient is not finite (a third-order solve on a Karras schedule's repeated last sigma,
        where ``step`` itself yields NaN)."""
        self._require_steps()
        if self._step_index is None:
            self._init_step_index(timestep)
        i, f = self._step_index, float
        p, q = _alpha_convert_pq(self.config.prediction_type, self.predict_x0, *self._alpha_sigma())
        row = [p, q] + [0.0] * 10
        with np.errstate(divide="ignore", invalid="ignore"):
            if self._use_corrector():
                o = self.this_order
                A, B, G, rks, rhos = self._bh_scalars(i, i - 1, [i - (k + 1) for k in range(1, o)], o, corrector=True)
                row[2], row[3], row[6], row[11] = f(A), -f(B), -f(G) * f(rhos[-1]), 1.0
                for k, rk in enumerate(rks):
                    row[4 + k] = -f(G) * f(rhos[k]) / f(rk)
            self.this_order = o = self._next_order()
            A, B, G, rks, rhos = self._bh_scalars(i + 1, i, [i - k for k in range(1, o)], o, corrector=False)
            row[7], row[8] = f(A), -f(B)
            for k, rk in enumerate(rks):
                row[9 + k] = -f(G) * f(rhos[k]) / f(rk)
        if self.last_sample is None:
            self.last_sample = _WALKED
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1
        if not all(map(isfinite, row)):
            raise NotImplementedError("a UniPC coefficient of this step is not finite")
        return tuple(row)

    def add_noise(self, original_samples, noise, timesteps):   # (not _Schedule's: the CURRENT schedule's sigmas, not the table)
        """:822-843: alpha_t x + sigma_t noise with the sigma of each timestep's index in the CURRENT schedule"""
        ts = np.atleast_1d(np.asarray(timesteps.detach().cpu() if torch.is_tensor(timesteps) else timesteps)).astype(np.int64)
        idx = [int(np.nonzero(self.timesteps == t)[0].item()) for t in ts]
        alpha_t, sigma_t = self._sigma_to_alpha_sigma_t(np.asarray(self.sigmas, dtype=np.float32)[idx])
        alpha_t = torch.as_tensor(alpha_t).to(original_samples.device, original_samples.dtype)
        sigma_t = torch.as_tensor(sigma_t).to(original_samples.device, original_samples.dtype)
        while alpha_t.dim() < original_samples.dim():
            alpha_t, sigma_t = alpha_t.unsqueeze(-1), sigma_t.unsqueeze(-1)
        return alpha_t * original_samples + sigma_t * noise


class DPMSolverSinglestepScheduler(_Schedule):
    """The singlestep DPM-Solver(++) of orders 1-3 (scheduling_dpmsolver_singlestep.py:75-920; what diffusers-style front ends pick
    for their "DPM++ 2S"-type presets): the evaluations run in groups of ``solver_order``, an order-k evaluation stepping from the
    sample parked k - 1 evaluations earlier with the group's converted outputs as differences against its first. Implemented:
    ``solver_order`` 1-3, "dpmsolver++" / "dpmsolver" ("deis" becomes "dpmsolver++"), "midpoint" / "heun" ("logrho" / "bh1" / "bh2"
    become "midpoint"), epsilon / sample / v_prediction, ``lower_order_final`` (switched on by ``set_timesteps`` when the step count is
    no multiple of the order), Karras sigmas, the img2img order reduction of ``step``. linspace spacing only, as the reference.
    Not implemented (NotImplementedError): thresholding, ``trained_betas``, a finite ``lambda_min_clipped``, ``variance_type``.

    The step's scalars are float32 TENSOR expressions, as the reference's 0-dim tensors give them, not numpy's as in
    ``DPMSolverMultistepScheduler._update_scalars``: numpy's float32 log and exp round differently from the tensor library's on one
    argument in eight, this update divides differences of logs by each other, and the recorded loops
    (tests/golden/singlestep) are reproduced bit for bit only with the tensor ones. The training table is the "tensor" one for the
    same reason. Every evaluation is linear in the tensors: ``singlestep_coefficients`` returns it as one row for the library's
    ``mi355x_sd_singlestep_update``."""

    _train_arithmetic = "tensor"

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", trained_betas=None, solver_order: int = 2, prediction_type: str = "epsilon",
                 thresholding: bool = False, dynamic_thresholding_ratio: float = 0.995, sample_max_value: float = 1.0,
                 algorithm_type: str = "dpmsolver++", solver_type: str = "midpoint", lower_order_final: bool = True,
                 use_karras_sigmas: Optional[bool] = False, lambda_min_clipped: float = -float("inf"),
                 variance_type: Optional[str] = None):
        if algorithm_type not in ("dpmsolver", "dpmsolver++"):
            if algorithm_type != "deis":
                raise NotImplementedError(f"{algorithm_type} does is not implemented for {self.__class__}")
            algorithm_type = "dpmsolver++"
        if solver_type not in ("midpoint", "heun"):
            if solver_type not in ("logrho", "bh1", "bh2"):
                raise NotImplementedError(f"{solver_type} does is not implemented for {self.__class__}")
            solver_type = "midpoint"
        self._capture(locals())
        if solver_order not in (1, 2, 3) or thresholding or lambda_min_clipped != -float("inf") or variance_type:
            raise NotImplementedError("DPMSolverSinglestepScheduler(mi355x): solver_order outside 1-3, thresholding, "
                                      "lambda_min_clipped and learned variance are not implemented")
        self._build()
        self.order_list = self.get_order_list(num_train_timesteps)

    def _reset(self):
        self.model_outputs = [None] * self.config.solver_order
        self.sample = None
        self._last_order = 0   # the effective order of the evaluation before this one (0: none yet)
        self._step_index = None

    coefficient_walk = _coefficient_walk("_step_index", "model_outputs", "sample", "_last_order")   # (singlestep_coefficients)

    def get_order_list(self, num_inference_steps: int):
        """the solver order listed for each step (:201-233)"""
        steps, order = num_inference_steps, self.config.solver_order
        if order == 1:
            return [1] * steps
        if not self.config.lower_order_final:
            return list(range(1, order + 1)) * (steps // order)
        if order == 2:
            return [1, 2] * (steps // 2) + [1] * (steps % 2)
        if steps % 3 == 0:
            return [1, 2, 3] * (steps // 3 - 1) + [1, 2] + [1]
        return [1, 2, 3] * (steps // 3) + ([1] if steps % 3 == 1 else [1, 2])

    def set_timesteps(self, num_inference_steps: int):
        c = self.config
        spaced = SimpleNamespace(timestep_spacing="linspace", steps_offset=0, num_train_timesteps=c.num_train_timesteps,
                                 use_karras_sigmas=c.use_karras_sigmas)   # (the reference has this one spacing and no offset)
        self.sigmas, self.timesteps = _multistep_schedule(self.alphas_cumprod, spaced, num_inference_steps, karras_ends_as_float=True)
        self.num_inference_steps = num_inference_steps
        if not c.lower_order_final and num_inference_steps % c.solver_order != 0:
            c.lower_order_final = True   # (:287-291: an uneven step count is finished at lower order, from now on)
        self.order_list = self.get_order_list(num_inference_steps)
        self._reset()

    _init_step_index = _init_multistep_index
    _sigma_to_alpha_sigma_t = staticmethod(_sigma_to_alpha_sigma_t)
    add_noise = UniPCMultistepScheduler.add_noise   # (:896-917: the CURRENT schedule's sigmas, as UniPC's)

    def _alpha_sigma(self) -> Tuple[float, float]:
        _check_alpha_prediction_type(self.config.prediction_type, "DPMSolverSinglestepScheduler")
        return _alpha_sigma_floats(torch.from_numpy(self.sigmas)[self._step_index])

    def convert_model_output(self, model_output, *args, sample=None, **kwargs):
        """model output -> x0 prediction (dpmsolver++) or epsilon prediction (dpmsolver), :393-480"""
        if sample is None:
            if len(args) < 2:
                raise ValueError("missing `sample` as a required keyward argument")
            sample = args[1]
        c = self.config
        return _alpha_convert(c.prediction_type, c.algorithm_type == "dpmsolver++", *self._alpha_sigma(), sample, model_output)

    def _effective_order(self, have) -> int:
        """the order listed for this step, lowered until the group has that many outputs (:859-864: an img2img loop may start where
        the list says 2 or 3). `have`: the converted outputs held, this step's included, oldest first; None = not there"""
        order = self.order_list[self._step_index]
        while have[-order] is None:
            order -= 1
        return order

    def _update_scalars(self, order: int):
        """The scalars of an order-`order` update that ends at sigma index ``_step_index + 1`` and starts `order` - 1 indices before
        ``_step_index`` -> (A, b, terms), each a float of a float32 tensor expression:
            order 1 (:526-536)   prev = A x - b m0                                             terms = ()
            order 2 (:583-630)   D1 = ri0 (m0 - m1);  prev = A S - b m1 -/+ c D1                terms = (ri0, c, plus)
            order 3, midpoint    D1_1 = ri0 (m0 - m2);  prev = A S - b m2 -/+ c D1_1            terms = (ri0, c, plus)
            order 3, heun        D1_0 = ri1 (m1 - m2), D1 = (r0 D1_0 - r1 D1_1) / (r0 - r1), D2 = 2 (D1_1 - D1_0) / (r0 - r1);
                                 prev = A S - b m2 -/+ c D1 - d D2                              terms = (ri0, c, plus, ri1, r0, r1, r01, d)
        ri0 = 1 / r0, ri1 = 1 / r1, r01 = r0 - r1. ``step`` and ``singlestep_coefficients`` both read this and nothing else of the
        schedule. c and d come with the sign the reference's expressions give them and `plus` apart, as in the multistep class."""
        cfg, i, f = self.config, self._step_index, float
        sig = torch.from_numpy(self.sigmas)
        lam = lambda a, s: torch.log(a) - torch.log(s)   # noqa: E731
        at, st = _sigma_to_alpha_sigma_t(sig[i + 1])
        a0, s0 = _sigma_to_alpha_sigma_t(sig[i])
        ab, sb = _sigma_to_alpha_sigma_t(sig[i - (order - 1)])   # where the group started: s0 (order 1), s1, s2
        lt, l0, lb = lam(at, st), lam(a0, s0), lam(ab, sb)
        h = lt - lb
        pp = cfg.algorithm_type == "dpmsolver++"
        A, b = (f(st / sb), f(at * (torch.exp(-h) - 1.0))) if pp else (f(at / ab), f(st * (torch.exp(h) - 1.0)))
        if order == 1:
            return A, b, ()
        r0 = (l0 - lb) / h
        heun = cfg.solver_type == "heun"
        first = at * ((torch.exp(-h) - 1.0) / h + 1.0) if pp else st * ((torch.exp(h) - 1.0) / h - 1.0)
        if order == 2 and not heun:
            return A, b, (f(1.0 / r0), f(0.5 * (at * (torch.exp(-h) - 1.0))) if pp else f(0.5 * (st * (torch.exp(h) - 1.0))), False)
        if order == 2 or not heun:
            return A, b, (f(1.0 / r0), f(first), pp)
        a1, s1 = _sigma_to_alpha_sigma_t(sig[i - 1])
        r1 = (lam(a1, s1) - lb) / h
        d = at * ((torch.exp(-h) - 1.0 + h) / h ** 2 - 0.5) if pp else st * ((torch.exp(h) - 1.0 - h) / h ** 2 - 0.5)
        return A, b, (f(1.0 / r0), f(first), pp, f(1.0 / r1), f(r0), f(r1), f(r0 - r1), f(d))

    def step(self, model_output, timestep, sample, return_dict: bool = True):
        self._require_steps()
        if self._step_index is None:
            self._init_step_index(timestep)
        m0 = self.convert_model_output(model_output, sample=sample)
        self.model_outputs = self.model_outputs[1:] + [m0]
        order = self._effective_order(self.model_outputs)
        if order == 1:   # "for single-step solvers, we use the initial value at each time with order = 1"
            self.sample = sample
        A, b, terms = self._update_scalars(order)
        base = self.model_outputs[-order]
        prev = A * self.sample - b * base
        if len(terms) == 3:
            ri0, c, plus = terms
            d1 = ri0 * (m0 - base)
            prev = prev + c * d1 if plus else prev - c * d1
        elif terms:
            ri0, c, plus, ri1, r0, r1, r01, d = terms
            d1_0, d1_1 = ri1 * (self.model_outputs[-2] - base), ri0 * (m0 - base)
            d1 = (r0 * d1_0 - r1 * d1_1) / r01
            d2 = 2.0 * (d1_1 - d1_0) / r01
            prev = (prev + c * d1 if plus else prev - c * d1) - d * d2
        self._last_order = order
        self._step_index += 1
        return _out(prev, return_dict)

    def singlestep_coefficients(self, timestep) -> Tuple[float, ...]:
        """This model evaluation as a linear map of the sample x the loop holds, the model output e, the parked sample S and the
        converted outputs of the evaluation's group, ``base`` its first and m1 its second -> (p, q, A, B, E1, E2, order, keep):
            m0   = p x + q e                                      (``convert_model_output``)
            prev = A x + B m0                                     order 1; afterwards S = x and base = m0
            prev = A S + B base + E1 (m0 - base)                  order 2; afterwards m1 = m0 where keep = 1.0 (order 3 follows)
            prev = A S + B base + E1 (m0 - base) + E2 (m1 - base) order 3; E2 = 0.0 for "midpoint"
        ``order`` is the EFFECTIVE order, after the reduction of ``step``. Advances ``_step_index``, ``model_outputs`` (placeholders
        for the tensors) and ``sample`` as ``step`` does. The schedule values are ``_update_scalars``' and the alpha_t, sigma_t of
        ``convert_model_output``, the very numbers ``step`` reads; the row is composed from them in float64.
        An effective order k > 1 directly follows effective order k - 1: every order list is made of runs 1, 2, .. and the reduction
        lowers an order to the number of outputs held, which is one more than it was an evaluation earlier. The device planes rely
        on it (the parked sample and ``base`` are what the order-1 evaluation of the group left, m1 what its order-2 one left), so it
        is checked here. NotImplementedError: that invariant broken, a history that holds tensors (``step`` has run on this
        scheduler: the planes never saw them), thresholding switched on, a coefficient that is not finite; the step state is then
        what it was before the call."""
        self._require_steps()
        fresh = self._step_index is None
        if fresh:
            self._init_step_index(timestep)
        try:
            return self._walk_row()
        except NotImplementedError:
            if fresh:
                self._step_index = None
            raise

    def _walk_row(self):
        cfg = self.config
        if cfg.thresholding or cfg.prediction_type not in ("epsilon", "sample", "v_prediction"):
            raise NotImplementedError("the fused form has no thresholding, and is for epsilon, sample or v prediction")
        if any(m is not None and m is not _WALKED for m in self.model_outputs):
            raise NotImplementedError("the history of this scheduler was not built by a coefficient walk")
        have = self.model_outputs[1:] + [_WALKED]
        order = self._effective_order(have)
        if order > 1 and self._last_order != order - 1:
            raise NotImplementedError(f"an order-{order} evaluation that does not follow an order-{order - 1} one")
        p, q = _alpha_convert_pq(cfg.prediction_type, cfg.algorithm_type == "dpmsolver++", *self._alpha_sigma())
        with np.errstate(divide="ignore", invalid="ignore"):
            A, b, terms = self._update_scalars(order)
            E1 = E2 = 0.0
            try:
                if len(terms) == 3:
                    ri0, c, plus = terms
                    E1 = (c if plus else -c) * ri0
                elif terms:
                    ri0, c, plus, ri1, r0, r1, r01, d = terms
                    sc = c if plus else -c
                    E1 = (sc * (-r1 * ri0) - d * 2.0 * ri0) / r01
                    E2 = (sc * (r0 * ri1) + d * 2.0 * ri1) / r01
            except ZeroDivisionError:
                E1 = float("nan")
        nxt = self._step_index + 1
        keep = float(order == 2 and nxt < len(self.order_list) and self.order_list[nxt] == 3)
        row = (p, q, A, -b, E1, E2, float(order), keep)
        if not all(map(isfinite, row)):
            raise NotImplementedError("a singlestep coefficient of this evaluation is not finite")
        self.model_outputs = have
        if order == 1:
            self.sample = _WALKED
        self._last_order = order
        self._step_index += 1
        return row


class FlowMatchEulerDiscreteScheduler:
    order = 1

    def __init__(self, num_train_timesteps: int = 1000, shift: float = 1.0):
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, shift=shift)
        ts = np.linspace(1, num_train_timesteps, num_train_timesteps, dtype=np.float32)[::-1].copy()
        sig = ts / num_train_timesteps
        sig = shift * sig / (1 + (shift - 1) * sig)
        self.sigmas = sig.astype(np.float32)
        self.timesteps = self.sigmas * num_train_timesteps
        self.sigma_min, self.sigma_max = float(self.sigmas[-1]), float(self.sigmas[0])
        self._step_index = None
        self.init_noise_sigma = 1.0

    def set_timesteps(self, num_inference_steps: int):
        T, shift = self.config.num_train_timesteps, self.config.shift
        ts = np.linspace(self.sigma_max * T, self.sigma_min * T, num_inference_steps)
        sig = ts / T
        sig = (shift * sig / (1 + (shift - 1) * sig)).astype(np.float32)
        self.timesteps = sig * T
        self.sigmas = np.concatenate([sig, np.zeros(1, np.float32)])
        self.num_inference_steps = num_inference_steps
        self._step_index = None

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step(self, model_output, timestep, sample, return_dict: bool = True, **unused):
        if self._step_index is None:
            idx = np.nonzero(self.timesteps == np.float32(float(timestep)))[0]
            self._step_index = int(idx[1] if len(idx) > 1 else idx[0])
        s, s_next = float(self.sigmas[self._step_index]), float(self.sigmas[self._step_index + 1])
        prev = (sample.to(torch.float32) + (s_next - s) * model_output.to(torch.float32)).to(model_output.dtype)
        self._step_index += 1
        return _out(prev, return_dict)


class LCMScheduler(_Schedule):
    """Multistep consistency sampling for latent-consistency models / LCM-LoRA (scheduling_lcm.py:140-631): the schedule is a
    subset of the ``original_inference_steps`` distillation schedule, each step predicts x0, applies the boundary-condition
    scalings (c_skip, c_out) and -- except on the last step -- re-noises to the next timestep with fresh noise."""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", original_inference_steps: int = 50, clip_sample: bool = False,
                 clip_sample_range: float = 1.0, set_alpha_to_one: bool = True, steps_offset: int = 0,
                 prediction_type: str = "epsilon", timestep_spacing: str = "leading", timestep_scaling: float = 10.0):
        self._capture(locals())
        self.custom_timesteps = False
        self._build()

    def _reset(self):
        self._step_index = None

    def set_timesteps(self, num_inference_steps: Optional[int] = None, original_inference_steps: Optional[int] = None,
                      timesteps=None, strength: float = 1.0):
        c = self.config
        if num_inference_steps is None and timesteps is None:
            raise ValueError("Must pass exactly one of `num_inference_steps` or `custom_timesteps`.")
        if num_inference_steps is not None and timesteps is not None:
            raise ValueError("Can only pass one of `num_inference_steps` or `custom_timesteps`.")
        original_steps = original_inference_steps if original_inference_steps is not None else c.original_inference_steps
        if original_steps > c.num_train_timesteps:
            raise ValueError(f"`original_steps`: {original_steps} cannot be larger than `self.config.train_timesteps`: "
                             f"{c.num_train_timesteps}")
        k = c.num_train_timesteps // original_steps                        # the paper's skipping step
        origin = np.arange(1, int(original_steps * strength) + 1) * k - 1    # distillation schedule, ascending
        if timesteps is not None:
            ts = np.array(timesteps, dtype=np.int64)
            if np.any(ts[1:] >= ts[:-1]):
                raise ValueError("`custom_timesteps` must be in descending order.")
            if ts[0] >= c.num_train_timesteps:
                raise ValueError(f"`timesteps` must start before `self.config.train_timesteps`: {c.num_train_timesteps}.")
            self.num_inference_steps, self.custom_timesteps = len(ts), True
            init = min(int(self.num_inference_steps * strength), self.num_inference_steps)
            ts = ts[max(self.num_inference_steps - init, 0) * self.order:]
        else:
            if num_inference_steps > c.num_train_timesteps:
                raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                                 f"`self.config.train_timesteps`: {c.num_train_timesteps}")
            if len(origin) // num_inference_steps < 1:
                raise ValueError(f"The combination of `original_steps x strength`: {original_steps} x {strength} is smaller "
                                 f"than `num_inference_steps`: {num_inference_steps}.")
            if num_inference_steps > original_steps:
                raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                                 f"`original_inference_steps`: {original_steps}")
            self.num_inference_steps, self.custom_timesteps = num_inference_steps, False
            rev = origin[::-1]
            idx = np.floor(np.linspace(0, len(rev), num=num_inference_steps, endpoint=False)).astype(np.int64)
            ts = rev[idx]
        self.timesteps = ts.astype(np.int64)
        self._reset()

    def _init_step_index(self, timestep):   # (not _Schedule's: a timestep outside the schedule is an IndexError here)
        idx = np.nonzero(self.timesteps == int(timestep))[0]
        self._step_index = int(idx[1] if len(idx) > 1 else idx[0])

    def get_scalings_for_boundary_condition_discrete(self, timestep):
        sigma_data = 0.5
        st = float(timestep) * self.config.timestep_scaling
        return sigma_data ** 2 / (st ** 2 + sigma_data ** 2), st / (st ** 2 + sigma_data ** 2) ** 0.5

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True, *, noise=None):
        """-> prev_sample (and ``denoised``, the x0 estimate the LCM pipeline decodes). ``noise`` (extension): the re-noising
        draw, otherwise ``torch.randn`` from ``generator``."""
        self._require_steps()
        if self._step_index is None:
            self._init_step_index(timestep)
        c, t = self.config, int(timestep)
        nxt = self._step_index + 1
        prev_t = int(self.timesteps[nxt]) if nxt < len(self.timesteps) else t
        a_t = float(self.alphas_cumprod[t])
        a_prev = float(self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod)
        c_skip, c_out = self.get_scalings_for_boundary_condition_discrete(t)
        if c.prediction_type == "epsilon":
            x0 = (sample - (1 - a_t) ** 0.5 * model_output) / a_t ** 0.5
        elif c.prediction_type == "sample":
            x0 = model_output
        elif c.prediction_type == "v_prediction":
            x0 = a_t ** 0.5 * sample - (1 - a_t) ** 0.5 * model_output
        else:
            raise ValueError(f"prediction_type given as {c.prediction_type} must be one of `epsilon`, `sample` or "
                             "`v_prediction` for `LCMScheduler`.")
        if c.clip_sample:
            x0 = x0.clamp(-c.clip_sample_range, c.clip_sample_range)
        denoised = c_out * x0 + c_skip * sample
        if self._step_index != self.num_inference_steps - 1:
            if noise is None:
                noise = torch.randn(model_output.shape, generator=generator, device=model_output.device,
                                    dtype=denoised.dtype)
            prev = a_prev ** 0.5 * denoised + (1 - a_prev) ** 0.5 * noise
        else:
            prev = denoised
        self._step_index += 1
        if not return_dict:
            return (prev, denoised)
        return SimpleNamespace(prev_sample=prev, denoised=denoised)

    def _table_index(self, timesteps):
        return torch.as_tensor(timesteps).long().cpu()   # (the other classes index the table with the timesteps as they come)
