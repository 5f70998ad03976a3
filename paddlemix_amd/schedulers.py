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
"""
from __future__ import annotations

from contextlib import contextmanager
from types import SimpleNamespace
from typing import Optional, Tuple

import numpy as np
import torch


def _make_betas(n: int, beta_start: float, beta_end: float, schedule: str) -> np.ndarray:
    if schedule == "linear":
        return np.linspace(beta_start, beta_end, n, dtype=np.float32)
    if schedule == "scaled_linear":  # the latent-diffusion schedule
        return np.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=np.float32) ** 2
    raise NotImplementedError(f"{schedule} is not implemented")


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


class DDIMScheduler:
    order = 1

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", clip_sample: bool = True, set_alpha_to_one: bool = True,
                 steps_offset: int = 0, prediction_type: str = "epsilon", clip_sample_range: float = 1.0,
                 timestep_spacing: str = "leading"):
        self.config = SimpleNamespace(**{k: v for k, v in locals().items() if k != "self"})
        betas = _make_betas(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.alphas_cumprod = np.cumprod(1.0 - betas, dtype=np.float32)
        self.final_alpha_cumprod = np.float32(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps: int):
        c = self.config
        if num_inference_steps > c.num_train_timesteps:
            raise ValueError("`num_inference_steps` cannot be larger than `num_train_timesteps`")
        self.num_inference_steps = num_inference_steps
        if c.timestep_spacing == "leading":
            step_ratio = c.num_train_timesteps // num_inference_steps
            ts = (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy().astype(np.int64)
            ts += c.steps_offset
        elif c.timestep_spacing == "trailing":
            ts = np.round(np.arange(c.num_train_timesteps, 0, -c.num_train_timesteps / num_inference_steps))
            ts = ts.astype(np.int64) - 1
        elif c.timestep_spacing == "linspace":
            ts = np.linspace(0, c.num_train_timesteps - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
        else:
            raise ValueError(f"{c.timestep_spacing} is not supported")
        self.timesteps = ts

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
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating "
                             "the scheduler")
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

    def add_noise(self, original_samples, noise, timesteps):
        a = torch.as_tensor(self.alphas_cumprod)[timesteps].to(original_samples.device)
        while a.dim() < original_samples.dim():
            a = a.unsqueeze(-1)
        return a ** 0.5 * original_samples + (1 - a) ** 0.5 * noise

    def __len__(self):
        return self.config.num_train_timesteps


class PNDMScheduler:
    """Pseudo numerical methods for diffusion models: Runge-Kutta warm-up (``step_prk``) + linear multistep (``step_plms``);
    Stable Diffusion uses ``skip_prk_steps=True`` (crowsonkb's PLMS, scheduling_pndm.py:216-223)."""
    order = 1

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", skip_prk_steps: bool = False, set_alpha_to_one: bool = False,
                 prediction_type: str = "epsilon", timestep_spacing: str = "leading", steps_offset: int = 0):
        self.config = SimpleNamespace(**{k: v for k, v in locals().items() if k != "self"})
        betas = _make_betas(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.alphas_cumprod = np.cumprod(1.0 - betas, dtype=np.float32)
        self.final_alpha_cumprod = np.float32(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.pndm_order = 4
        self.cur_model_output, self.counter, self.cur_sample, self.ets = 0, 0, None, []
        self.num_inference_steps = None
        self._timesteps = np.arange(0, num_train_timesteps)[::-1].copy()
        self.prk_timesteps = self.plms_timesteps = self.timesteps = None

    def set_timesteps(self, num_inference_steps: int):
        c = self.config
        self.num_inference_steps = n = num_inference_steps
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, c.num_train_timesteps - 1, n).round().astype(np.int64)
        elif c.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (c.num_train_timesteps // n)).round().astype(np.int64) + c.steps_offset
        elif c.timestep_spacing == "trailing":
            ts = np.round(np.arange(c.num_train_timesteps, 0, -c.num_train_timesteps / n))[::-1].astype(np.int64) - 1
        else:
            raise ValueError(f"{c.timestep_spacing} is not supported. Please make sure to choose one of 'linspace', "
                             "'leading' or 'trailing'.")
        self._timesteps = ts
        if c.skip_prk_steps:
            self.prk_timesteps = np.array([], dtype=np.int64)
            self.plms_timesteps = np.concatenate([ts[:-1], ts[-2:-1], ts[-1:]])[::-1].copy()
        else:
            prk = np.array(ts[-self.pndm_order:]).repeat(2) + np.tile(np.array([0, c.num_train_timesteps // n // 2]),
                                                                        self.pndm_order)
            self.prk_timesteps = (prk[:-1].repeat(2)[1:-1])[::-1].copy()
            self.plms_timesteps = ts[:-3][::-1].copy()
        self.timesteps = np.concatenate([self.prk_timesteps, self.plms_timesteps]).astype(np.int64)
        self.ets, self.counter, self.cur_model_output = [], 0, 0

    def scale_model_input(self, sample, *args, **kwargs):
        return sample

    def step(self, model_output, timestep, sample, return_dict: bool = True):
        if self.counter < len(self.prk_timesteps) and not self.config.skip_prk_steps:
            return self.step_prk(model_output, timestep, sample, return_dict)
        return self.step_plms(model_output, timestep, sample, return_dict)

    def _require_steps(self):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")

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
        step = self.config.num_train_timesteps // self.num_inference_steps
        timestep = int(timestep)
        prev_timestep = timestep - step
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(model_output)
        else:
            prev_timestep, timestep = timestep, timestep + step
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

    def _get_prev_sample(self, sample, timestep, prev_timestep, model_output):
        """formula (9) of the PNDM paper (scheduling_pndm.py:410-453), coefficients in float32 like the reference's tables"""
        a_t = self.alphas_cumprod[timestep]
        a_prev = self.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        b_t, b_prev = 1 - a_t, 1 - a_prev
        if self.config.prediction_type == "v_prediction":
            model_output = float(a_t ** 0.5) * model_output + float(b_t ** 0.5) * sample
        elif self.config.prediction_type != "epsilon":
            raise ValueError(f"prediction_type given as {self.config.prediction_type} must be one of `epsilon` or `v_prediction`")
        coeff = float((a_prev / a_t) ** 0.5)
        denom = a_t * b_prev ** 0.5 + (a_t * b_t * a_prev) ** 0.5
        return coeff * sample - float((a_prev - a_t) / denom) * model_output

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
        ``cur_sample``). t and t_prev are derived from ``timestep`` and ``counter`` as ``step_plms`` derives them, so a loop that starts
        inside the schedule gets that method's own second evaluation. Every schedule value is the float32 numpy expression of
        ``_get_prev_sample``; the weights are the exact rationals. NotImplementedError: the Runge-Kutta warm-up (``skip_prk_steps=False``),
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
        step = cfg.num_train_timesteps // self.num_inference_steps
        t = int(timestep)
        t_prev = t - step
        if c != 1:
            self.ets = self.ets[-3:] + [_WALKED]
        else:
            t_prev, t = t, t + step
        w = self._PLMS_WEIGHTS[(min(c, 4), len(self.ets))]
        self.cur_sample = _WALKED if c == 0 else None if c == 1 else self.cur_sample
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[t_prev] if t_prev >= 0 else self.final_alpha_cumprod
        b_t, b_prev = 1 - a_t, 1 - a_prev
        p, q = (float(b_t ** 0.5), float(a_t ** 0.5)) if cfg.prediction_type == "v_prediction" else (0.0, 1.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = float((a_prev / a_t) ** 0.5)
            denom = a_t * b_prev ** 0.5 + (a_t * b_t * a_prev) ** 0.5
            b = -float((a_prev - a_t) / denom)
        self.counter += 1
        row = (a, b, p, q) + w + (float(max(c - 1, 0) % 3) if c != 1 else 1.0, float(c == 0), float(c == 1), 0.0)
        if not all(np.isfinite(v) for v in row):
            raise NotImplementedError("a PLMS coefficient of this evaluation is not finite")
        return row

    def add_noise(self, original_samples, noise, timesteps):
        a = torch.as_tensor(self.alphas_cumprod)[timesteps].to(original_samples.device)
        while a.dim() < original_samples.dim():
            a = a.unsqueeze(-1)
        return a ** 0.5 * original_samples + (1 - a) ** 0.5 * noise

    def __len__(self):
        return self.config.num_train_timesteps


class EulerDiscreteScheduler:
    order = 1

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", prediction_type: str = "epsilon", interpolation_type: str = "linear",
                 use_karras_sigmas: bool = False, timestep_spacing: str = "linspace", steps_offset: int = 0):
        self.config = SimpleNamespace(**{k: v for k, v in locals().items() if k != "self"})
        betas = _make_betas(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.alphas_cumprod = np.cumprod(1.0 - betas, dtype=np.float32)
        self._train_sigmas = ((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5
        self.sigmas = np.concatenate([self._train_sigmas[::-1], [0.0]]).astype(np.float32)
        self.timesteps = np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=float)[::-1].astype(
            np.float32)
        self.num_inference_steps = None
        self._step_index: Optional[int] = None

    @property
    def init_noise_sigma(self):
        m = float(self.sigmas.max())
        if self.config.timestep_spacing in ("linspace", "trailing"):
            return m
        return (m ** 2 + 1) ** 0.5

    @property
    def step_index(self):
        return self._step_index

    coefficient_walk = _coefficient_walk("_step_index")   # (step_coefficients, model_input_scale)

    def set_timesteps(self, num_inference_steps: int):
        c = self.config
        self.num_inference_steps = n = num_inference_steps
        T = c.num_train_timesteps
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n, dtype=np.float32)[::-1].copy()
        elif c.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.float32) + c.steps_offset
        elif c.timestep_spacing == "trailing":
            ts = (np.arange(T, 0, -T / n)).round().copy().astype(np.float32) - 1
        else:
            raise ValueError(f"{c.timestep_spacing} is not supported")
        sig_all = np.array(self._train_sigmas)
        log_sig = np.log(sig_all)
        if c.interpolation_type == "linear":
            sig = np.interp(ts, np.arange(0, len(sig_all)), sig_all)
        elif c.interpolation_type == "log_linear":
            sig = np.exp(np.linspace(np.log(sig_all[-1]), np.log(sig_all[0]), n + 1))
        else:
            raise ValueError(f"{c.interpolation_type} is not implemented")
        if c.use_karras_sigmas:
            rho = 7.0
            lo, hi = sig[-1] ** (1 / rho), sig[0] ** (1 / rho)
            sig = (hi + np.linspace(0, 1, n) * (lo - hi)) ** rho
            ts = np.array([self._sigma_to_t(s, log_sig) for s in sig])
        self.sigmas = np.concatenate([sig, [0.0]]).astype(np.float32)
        self.timesteps = ts.astype(np.float32)
        self._step_index = None

    @staticmethod
    def _sigma_to_t(sigma, log_sigmas):
        log_sigma = np.log(np.maximum(sigma, 1e-10))
        dists = log_sigma - log_sigmas[:, np.newaxis]
        low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
        high_idx = low_idx + 1
        low, high = log_sigmas[low_idx], log_sigmas[high_idx]
        w = np.clip((low - log_sigma) / (low - high), 0, 1)
        return ((1 - w) * low_idx + w * high_idx).reshape(np.shape(sigma))

    def _init_step_index(self, timestep):
        t = float(timestep)
        idx = np.nonzero(self.timesteps == np.float32(t))[0]
        # "the sigma index that is taken for the **very** first step is always the second index" (duplicates)
        self._step_index = int(idx[1] if len(idx) > 1 else idx[0])

    def scale_model_input(self, sample, timestep):
        if self._step_index is None:
            self._init_step_index(timestep)
        return sample / ((float(self.sigmas[self._step_index]) ** 2 + 1) ** 0.5)

    def model_input_scale(self, timestep) -> float:
        if self._step_index is None:
            self._init_step_index(timestep)
        return 1.0 / ((float(self.sigmas[self._step_index]) ** 2 + 1) ** 0.5)

    def step_coefficients(self, timestep) -> Tuple[float, float]:
        """(a, b) with prev = a*sample + b*model_output for epsilon or v prediction, s_churn = 0; advances the index."""
        if self.config.prediction_type not in ("epsilon", "v_prediction"):
            raise NotImplementedError("linear-update form is for epsilon or v prediction")
        if self._step_index is None:
            self._init_step_index(timestep)
        s, s_next = float(self.sigmas[self._step_index]), float(self.sigmas[self._step_index + 1])
        self._step_index += 1
        if self.config.prediction_type == "v_prediction":
            # step(): x0 = x / (s^2 + 1) - v s / sqrt(s^2 + 1), so (x - x0) / s = x s / (s^2 + 1) + v / sqrt(s^2 + 1)
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
        if pt in ("original_sample", "sample"):
            x0 = model_output
        elif pt == "epsilon":
            x0 = sample - sigma_hat * model_output
        elif pt == "v_prediction":
            x0 = model_output * (-sigma / (sigma ** 2 + 1) ** 0.5) + (sample / (sigma ** 2 + 1))
        else:
            raise ValueError(f"prediction_type given as {pt} must be one of `epsilon`, or `v_prediction`")
        derivative = (sample - x0) / sigma_hat
        dt = float(self.sigmas[self._step_index + 1]) - sigma_hat
        prev = sample + derivative * dt
        self._step_index += 1
        return _out(prev, return_dict, pred_original_sample=x0)

    def add_noise(self, original_samples, noise, timesteps):
        """scheduling_euler_discrete.py:480-500: x + noise * sigma[index of each timestep in the current schedule]"""
        ts = np.atleast_1d(np.asarray(timesteps.detach().cpu() if torch.is_tensor(timesteps) else timesteps, dtype=np.float32))
        idx = [int(np.nonzero(self.timesteps == t)[0][0]) for t in ts]
        sigma = torch.as_tensor(np.asarray(self.sigmas, dtype=np.float32)[idx]).to(original_samples.device,
                                                                                  original_samples.dtype)
        while sigma.dim() < original_samples.dim():
            sigma = sigma.unsqueeze(-1)
        return original_samples + noise * sigma

    def __len__(self):
        return self.config.num_train_timesteps


class EulerAncestralDiscreteScheduler:
    """"Euler a" (scheduling_euler_ancestral_discrete.py:130-389): an Euler step down to sigma_down and fresh noise of sigma_up back
    up, every step. epsilon and v prediction, the three spacings; ``trained_betas`` is not implemented. The step is linear in the
    sample, the model output and the noise: ``ancestral_coefficients`` returns (a, b, c) with  prev = a*sample + b*model_output +
    c*noise  for the library's ``mi355x_sd_ancestral_update``."""
    order = 1

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", trained_betas=None, prediction_type: str = "epsilon",
                 timestep_spacing: str = "linspace", steps_offset: int = 0):
        self.config = SimpleNamespace(**{k: v for k, v in locals().items() if k != "self"})
        if trained_betas is not None:
            raise NotImplementedError("EulerAncestralDiscreteScheduler(mi355x): trained_betas is not implemented")
        # The training table in float32 TENSOR arithmetic, as the reference builds it (:141-161: linspace, cumprod and the sigmas are
        # float32 tensor operations). _make_betas' float64 linspace rounded to float32 ends 9 float32 steps away at sigma_max, and an
        # ancestral loop, whose every step divides by sigma^2, carries that into the latents (tests/golden/euler_ancestral/README.md)
        if beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        else:
            raise NotImplementedError(f"{beta_schedule} is not implemented")
        alphas_cumprod = torch.cumprod(1.0 - betas, 0)
        self.alphas_cumprod = alphas_cumprod.numpy()
        self._train_sigmas = (((1 - alphas_cumprod) / alphas_cumprod) ** 0.5).numpy()
        self.sigmas = np.concatenate([self._train_sigmas[::-1], [0.0]]).astype(np.float32)
        self.timesteps = np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=float)[::-1].astype(np.float32)
        self.num_inference_steps = None
        self._step_index: Optional[int] = None

    @property
    def init_noise_sigma(self):
        m = float(self.sigmas.max())
        if self.config.timestep_spacing in ("linspace", "trailing"):
            return m
        return (m ** 2 + 1) ** 0.5

    @property
    def step_index(self):
        return self._step_index

    coefficient_walk = _coefficient_walk("_step_index")   # (ancestral_coefficients, model_input_scale)

    def set_timesteps(self, num_inference_steps: int):
        c, T = self.config, self.config.num_train_timesteps
        self.num_inference_steps = n = num_inference_steps
        if c.timestep_spacing == "linspace":   # (not rounded)
            ts = np.linspace(0, T - 1, n, dtype=np.float32)[::-1].copy()
        elif c.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.float32) + c.steps_offset
        elif c.timestep_spacing == "trailing":
            ts = (np.arange(T, 0, -T / n)).round().copy().astype(np.float32) - 1
        else:
            raise ValueError(f"{c.timestep_spacing} is not supported. Please make sure to choose one of 'linspace', "
                             "'leading' or 'trailing'.")
        sig_all = np.array(self._train_sigmas)
        sig = np.interp(ts, np.arange(0, len(sig_all)), sig_all)
        self.sigmas = np.concatenate([sig, [0.0]]).astype(np.float32)
        self.timesteps = ts.astype(np.float32)
        self._step_index = None

    _init_step_index = EulerDiscreteScheduler._init_step_index
    scale_model_input = EulerDiscreteScheduler.scale_model_input
    model_input_scale = EulerDiscreteScheduler.model_input_scale
    add_noise = EulerDiscreteScheduler.add_noise

    def _check(self, timestep):
        pt = self.config.prediction_type
        if pt == "sample":
            raise NotImplementedError("prediction_type not implemented yet: sample")
        if pt not in ("epsilon", "v_prediction"):
            raise ValueError(f"prediction_type given as {pt} must be one of `epsilon`, or `v_prediction`")
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
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
        if self.config.prediction_type == "v_prediction":
            # step(): x0 = x / (s^2 + 1) - v s / sqrt(s^2 + 1), so (x - x0) / s = x s / (s^2 + 1) + v / sqrt(s^2 + 1)
            a, b = 1.0 + dt * s / (s ** 2 + 1), dt / (s ** 2 + 1) ** 0.5
        else:
            a, b = 1.0, dt
        if not all(np.isfinite(v) for v in (a, b, c)):
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
        if self.config.prediction_type == "epsilon":
            x0 = sample - s * model_output
        else:
            x0 = model_output * (-s / (s ** 2 + 1) ** 0.5) + (sample / (s ** 2 + 1))
        derivative = (sample - x0) / s
        prev = sample + derivative * dt
        if noise is None:
            noise = torch.randn(model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
        prev = prev + noise * s_up
        self._step_index += 1
        return _out(prev, return_dict, pred_original_sample=x0)

    def __len__(self):
        return self.config.num_train_timesteps


class HeunDiscreteScheduler:
    """"Heun" (scheduling_heun_discrete.py:71-480): the second-order k-diffusion sampler, two model evaluations per step. Every
    timestep but the first appears twice; the first evaluation of a pair takes an Euler step and parks the sample, the derivative and
    dt, the second averages the two derivatives and steps again from the parked sample; the last step (to sigma = 0) is a plain Euler
    step. epsilon, v_prediction and sample prediction, the three spacings, Karras sigmas, ``clip_sample``; ``trained_betas`` is not
    implemented. Both stages are linear in the current sample, the model output and the parked state: ``heun_coefficients`` returns
    (p, q, h, g, second) for the library's ``mi355x_sd_heun_update``."""
    order = 2

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "linear", trained_betas=None, prediction_type: str = "epsilon",
                 use_karras_sigmas: bool = False, clip_sample: bool = False, clip_sample_range: float = 1.0,
                 timestep_spacing: str = "linspace", steps_offset: int = 0):
        self.config = SimpleNamespace(**{k: v for k, v in locals().items() if k != "self"})
        if trained_betas is not None:
            raise NotImplementedError("HeunDiscreteScheduler(mi355x): trained_betas is not implemented")
        # the training table in float32 TENSOR arithmetic, as the reference builds it (:128-146) and as
        # EulerAncestralDiscreteScheduler does here (see there for what the float64 linspace of _make_betas costs)
        if beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        else:
            raise NotImplementedError(f"{beta_schedule} does is not implemented for {self.__class__}")
        alphas_cumprod = torch.cumprod(1.0 - betas, 0)
        self.alphas_cumprod = alphas_cumprod.numpy()
        self._train_sigmas = (((1 - alphas_cumprod) / alphas_cumprod) ** 0.5).numpy()
        self.use_karras_sigmas = use_karras_sigmas
        self.set_timesteps(num_train_timesteps)   # "set all values" (:149)

    @property
    def init_noise_sigma(self):
        m = np.float32(self.sigmas.max())
        if self.config.timestep_spacing in ("linspace", "trailing"):
            return float(m)
        return float(np.sqrt(m * m + np.float32(1.0)))   # float32, as the reference's tensor expression (max ** 2 + 1) ** 0.5

    @property
    def step_index(self):
        return self._step_index

    @property
    def state_in_first_order(self):
        return self.dt is None

    coefficient_walk = _coefficient_walk("_step_index", "dt")   # (heun_coefficients, model_input_scale)

    def set_timesteps(self, num_inference_steps: int):
        c, T = self.config, self.config.num_train_timesteps
        self.num_inference_steps = n = num_inference_steps
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n, dtype=np.float32)[::-1].copy()
        elif c.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.float32) + c.steps_offset
        elif c.timestep_spacing == "trailing":
            ts = (np.arange(T, 0, -T / n)).round().copy().astype(np.float32) - 1
        else:
            raise ValueError(f"{c.timestep_spacing} is not supported. Please make sure to choose one of 'linspace', "
                             "'leading' or 'trailing'.")
        sig_all = np.array(self._train_sigmas)
        log_sig = np.log(sig_all)
        sig = np.interp(ts, np.arange(0, len(sig_all)), sig_all)
        if c.use_karras_sigmas:   # (:304-327; the timesteps are not rounded)
            rho = 7.0
            lo, hi = sig[-1].item() ** (1 / rho), sig[0].item() ** (1 / rho)
            sig = (hi + np.linspace(0, 1, n) * (lo - hi)) ** rho
            ts = np.array([EulerDiscreteScheduler._sigma_to_t(s, log_sig) for s in sig])
        sig = np.concatenate([sig, [0.0]]).astype(np.float32)
        ts = ts.astype(np.float32)
        # [s0, s1, s1, ..., s_{n-1}, s_{n-1}, 0] and [t0, t1, t1, ..., t_{n-1}, t_{n-1}]: 2n sigmas, 2n - 1 timesteps
        self.sigmas = np.concatenate([sig[:1], np.repeat(sig[1:-1], 2), sig[-1:]])
        self.timesteps = np.concatenate([ts[:1], np.repeat(ts[1:], 2)])
        self.prev_derivative = self.dt = self.sample = None
        self._step_index: Optional[int] = None
        self._index_counter = {}

    def index_for_timestep(self, timestep, schedule_timesteps=None):
        """(:154-170) before any step: the second of two matching indices (the only one if single); afterwards the one the
        counter of ``step`` calls at this timestep points to"""
        ts = self.timesteps if schedule_timesteps is None else schedule_timesteps
        t = float(timestep)
        idx = np.nonzero(np.asarray(ts) == np.float32(t))[0]
        if len(self._index_counter) == 0:
            pos = 1 if len(idx) > 1 else 0
        else:
            pos = self._index_counter.setdefault(t, 0)
        return int(idx[pos])

    _init_step_index = EulerDiscreteScheduler._init_step_index

    def _sigma(self, i, dtype):
        """sigmas[i] as a 0-dim tensor of `dtype`: the reference casts its sigma tensor to the model output's dtype (:376-377), so the
        scalar expressions of ``step`` are rounded in that dtype"""
        return torch.tensor(float(self.sigmas[i]), dtype=dtype)

    def scale_model_input(self, sample, timestep):
        if self._step_index is None:
            self._init_step_index(timestep)
        sigma = self._sigma(self._step_index, sample.dtype)
        return sample / ((sigma ** 2 + 1) ** 0.5)

    def model_input_scale(self, timestep) -> float:
        if self._step_index is None:
            self._init_step_index(timestep)
        return 1.0 / ((float(self.sigmas[self._step_index]) ** 2 + 1) ** 0.5)

    def _check(self, timestep):
        pt = self.config.prediction_type
        if pt not in ("epsilon", "v_prediction", "sample"):
            raise ValueError(f"prediction_type given as {pt} must be one of `epsilon`, or `v_prediction`")
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
        pt = self.config.prediction_type
        with np.errstate(all="ignore"):
            s_in = np.float64(s_in)
            if pt == "epsilon":
                p, q = 0.0, 1.0
            elif pt == "v_prediction":
                # step(): x0 = x / (s^2 + 1) - v s / sqrt(s^2 + 1), so (x - x0) / s = x s / (s^2 + 1) + v / sqrt(s^2 + 1)
                p, q = float(s_in / (s_in ** 2 + 1)), float(1.0 / (s_in ** 2 + 1) ** 0.5)
            else:
                p, q = float(1.0 / s_in), float(-1.0 / s_in)
        if not all(np.isfinite(v) for v in (p, q, h)):
            raise NotImplementedError("a non-finite row has no linear-update form")
        return p, q, h, g, second

    def step(self, model_output, timestep, sample, return_dict: bool = True):
        """(:349-455) line by line; the sigmas enter as 0-dim tensors of the model output's dtype"""
        self._check(timestep)
        t = float(timestep)
        self._index_counter[t] = self._index_counter.get(t, 0) + 1
        i, dtype, c = self._step_index, model_output.dtype, self.config
        first = self.state_in_first_order
        if first:
            sigma, sigma_next = self._sigma(i, dtype), self._sigma(i + 1, dtype)
        else:   # 2nd order / Heun's method
            sigma, sigma_next = self._sigma(i - 1, dtype), self._sigma(i, dtype)
        sigma_hat = sigma   # gamma = 0
        sigma_input = sigma_hat if first else sigma_next
        if c.prediction_type == "epsilon":
            x0 = sample - sigma_input * model_output
        elif c.prediction_type == "v_prediction":
            x0 = model_output * (-sigma_input / (sigma_input ** 2 + 1) ** 0.5) + (sample / (sigma_input ** 2 + 1))
        else:
            x0 = model_output
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

    def add_noise(self, original_samples, noise, timesteps):
        """(:457-477) x + noise * sigma[index_for_timestep of each timestep]"""
        ts = np.atleast_1d(np.asarray(timesteps.detach().cpu() if torch.is_tensor(timesteps) else timesteps, dtype=np.float32))
        idx = [self.index_for_timestep(t) for t in ts]
        sigma = torch.as_tensor(np.asarray(self.sigmas, dtype=np.float32)[idx]).to(original_samples.device,
                                                                                  original_samples.dtype)
        while sigma.dim() < original_samples.dim():
            sigma = sigma.unsqueeze(-1)
        return original_samples + noise * sigma

    def __len__(self):
        return self.config.num_train_timesteps


class KDPM2DiscreteScheduler:
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

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "linear", trained_betas=None, use_karras_sigmas: bool = False,
                 prediction_type: str = "epsilon", timestep_spacing: str = "linspace", steps_offset: int = 0):
        self.config = SimpleNamespace(**{k: v for k, v in locals().items() if k != "self"})
        if trained_betas is not None:
            raise NotImplementedError(f"{self.__class__.__name__}(mi355x): trained_betas is not implemented")
        # the training table in float32 TENSOR arithmetic, as HeunDiscreteScheduler builds it
        if beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        else:
            raise NotImplementedError(f"{beta_schedule} does is not implemented for {self.__class__}")
        alphas_cumprod = torch.cumprod(1.0 - betas, 0)
        self.alphas_cumprod = alphas_cumprod.numpy()
        self._train_sigmas = (((1 - alphas_cumprod) / alphas_cumprod) ** 0.5).numpy()
        self.set_timesteps(num_train_timesteps, num_train_timesteps)   # "set all values" (:142)

    init_noise_sigma = HeunDiscreteScheduler.init_noise_sigma

    @property
    def step_index(self):
        return self._step_index

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
        c, T = self.config, num_train_timesteps or self.config.num_train_timesteps
        self.num_inference_steps = n = num_inference_steps
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n, dtype=np.float32)[::-1].copy()
        elif c.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.float32) + c.steps_offset
        elif c.timestep_spacing == "trailing":
            ts = (np.arange(T, 0, -T / n)).round().copy().astype(np.float32) - 1
        else:
            raise ValueError(f"{c.timestep_spacing} is not supported. Please make sure to choose one of 'linspace', "
                             "'leading' or 'trailing'.")
        sig_all = np.array(self._train_sigmas)
        log_sig = np.log(sig_all)
        sig = np.interp(ts, np.arange(0, len(sig_all)), sig_all)
        if c.use_karras_sigmas:   # (here the timesteps ARE rounded, :252)
            rho = 7.0
            lo, hi = sig[-1].item() ** (1 / rho), sig[0].item() ** (1 / rho)
            sig = (hi + np.linspace(0, 1, n) * (lo - hi)) ** rho
            ts = np.array([EulerDiscreteScheduler._sigma_to_t(s, log_sig) for s in sig]).round()
        sig = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        # entries no evaluation reads go through log(0) and inf - inf on the way, as in the reference
        tables, between = self._tables(sig)
        for k, v in dict(tables, sigmas=sig).items():   # [v0, v1, v1, ..., vn, vn, vn]: 2n + 2 entries
            setattr(self, k, torch.cat([v[:1], v[1:].repeat_interleave(2), v[-1:]]).numpy())
        with np.errstate(all="ignore"):
            # (one call over the array: the per-element arithmetic of the reference's loop over _sigma_to_t)
            t_interpol = EulerDiscreteScheduler._sigma_to_t(tables["sigmas_interpol"].numpy(), log_sig).astype(np.float32)
        ts = ts.astype(np.float32)
        # [t0, t'0, t1, t'1, ..., t_{n-1}]: 2n - 1 timesteps, t'k the timestep of the sigma stage 2 of step k is evaluated at
        self.timesteps = np.concatenate([ts[:1], np.stack((t_interpol[between], ts[1:]), axis=-1).reshape(-1)])
        self.sample = None
        self._step_index: Optional[int] = None
        self._index_counter = {}

    index_for_timestep = HeunDiscreteScheduler.index_for_timestep
    _init_step_index = EulerDiscreteScheduler._init_step_index
    add_noise = HeunDiscreteScheduler.add_noise

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

    def _check_prediction_type(self):
        pt = self.config.prediction_type
        if pt == "sample":
            raise NotImplementedError("prediction_type not implemented yet: sample")
        if pt not in ("epsilon", "v_prediction"):
            raise ValueError(f"prediction_type given as {pt} must be one of `epsilon`, or `v_prediction`")

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
        self._check_prediction_type()
        i, first = self._step_index, self.state_in_first_order
        s, s_interpol, s_to, s_up = (None if v is None else float(v) for v in self._stage(i, first))
        if first:
            s_in, h, c, second = s, s_interpol - s, 0.0, 0.0
            self.sample = _WALKED
        else:
            s_in, h, c, second = s_interpol, s_to - s, 0.0 if s_up is None else s_up, 1.0
            self.sample = None
        self._step_index += 1
        with np.errstate(all="ignore"):
            s_in = np.float64(s_in)
            if self.config.prediction_type == "epsilon":
                p, q = 0.0, 1.0
            else:   # step(): x0 = x / (s^2 + 1) - v s / sqrt(s^2 + 1), so (x - x0) / s = x s / (s^2 + 1) + v / sqrt(s^2 + 1)
                p, q = float(s_in / (s_in ** 2 + 1)), float(1.0 / (s_in ** 2 + 1) ** 0.5)
        if not all(np.isfinite(v) for v in (p, q, h, c)):
            raise NotImplementedError("a non-finite row has no linear-update form")
        return p, q, h, c, second

    def _begin(self, timestep):
        if self._step_index is None:
            self._init_step_index(timestep)
        t = float(timestep)
        self._index_counter[t] = self._index_counter.get(t, 0) + 1

    def _advance(self, model_output, sample, noise, return_dict):
        """(:411-462, ancestral :425-478) line by line from the prediction-type branch on"""
        i, dtype, first = self._step_index, model_output.dtype, self.state_in_first_order
        other = torch.promote_types(torch.float32, dtype)
        s, s_interpol, s_to, s_up = self._stage(i, first)
        sigma_hat = torch.tensor(float(s), dtype=dtype)   # gamma = 0
        sigma_interpol = torch.tensor(float(s_interpol), dtype=other)
        self._check_prediction_type()
        sigma_input = sigma_hat if first else sigma_interpol
        if self.config.prediction_type == "epsilon":
            x0 = sample - sigma_input * model_output
        else:
            x0 = model_output * (-sigma_input / (sigma_input ** 2 + 1) ** 0.5) + (sample / (sigma_input ** 2 + 1))
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

    def __len__(self):
        return self.config.num_train_timesteps


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


class DPMSolverMultistepScheduler:
    """The fast multistep solver most SD pipelines switch to (20-25 steps; the reference's DiT example uses it). Implemented:
    ``algorithm_type`` "dpmsolver++" / "dpmsolver", ``solver_order`` 1-2, "midpoint" / "heun", epsilon / v_prediction / sample,
    ``lower_order_final``, ``euler_at_final``, Karras sigmas. Not implemented (NotImplementedError): the SDE variants,
    third order, thresholding, ``use_lu_lambdas``, a finite ``lambda_min_clipped``."""
    order = 1

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", solver_order: int = 2, prediction_type: str = "epsilon",
                 thresholding: bool = False, dynamic_thresholding_ratio: float = 0.995, sample_max_value: float = 1.0,
                 algorithm_type: str = "dpmsolver++", solver_type: str = "midpoint", lower_order_final: bool = True,
                 euler_at_final: bool = False, use_karras_sigmas: bool = False, use_lu_lambdas: bool = False,
                 lambda_min_clipped: float = -float("inf"), variance_type: Optional[str] = None,
                 timestep_spacing: str = "linspace", steps_offset: int = 0):
        self.config = SimpleNamespace(**{k: v for k, v in locals().items() if k != "self"})
        if algorithm_type not in ("dpmsolver", "dpmsolver++"):
            raise NotImplementedError(f"{algorithm_type} is not implemented for {self.__class__}")
        if solver_type not in ("midpoint", "heun"):
            raise NotImplementedError(f"{solver_type} is not implemented for {self.__class__}")
        if solver_order not in (1, 2) or thresholding or use_lu_lambdas or lambda_min_clipped != -float("inf") or variance_type:
            raise NotImplementedError("DPMSolverMultistepScheduler(mi355x): solver_order 3, thresholding, use_lu_lambdas, "
                                      "lambda_min_clipped and learned variance are not implemented")
        betas = _make_betas(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.alphas_cumprod = np.cumprod(1.0 - betas, dtype=np.float32)
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=np.float32)[::-1].copy().astype(np.int64)
        self.model_outputs = [None] * solver_order
        self.lower_order_nums = 0
        self._step_index = None

    @property
    def step_index(self):
        return self._step_index

    coefficient_walk = _coefficient_walk("_step_index", "lower_order_nums", "model_outputs")   # (multistep_coefficients)

    def set_timesteps(self, num_inference_steps: int):
        c, n = self.config, num_inference_steps
        last = c.num_train_timesteps
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, last - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif c.timestep_spacing == "leading":
            ts = (np.arange(0, n + 1) * (last // (n + 1))).round()[::-1][:-1].copy().astype(np.int64) + c.steps_offset
        elif c.timestep_spacing == "trailing":
            ts = np.arange(last, 0, -c.num_train_timesteps / n).round().copy().astype(np.int64) - 1
        else:
            raise ValueError(f"{c.timestep_spacing} is not supported. Please make sure to choose one of 'linspace', "
                             "'leading' or 'trailing'.")
        sigmas = np.array(((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5)
        log_sigmas = np.log(sigmas)
        if c.use_karras_sigmas:
            s = np.flip(sigmas).copy()
            rho, ramp = 7.0, np.linspace(0, 1, n)
            s = (s[0] ** (1 / rho) + ramp * (s[-1] ** (1 / rho) - s[0] ** (1 / rho))) ** rho
            ts = np.array([EulerDiscreteScheduler._sigma_to_t(x, log_sigmas) for x in s]).round()
            sigmas = np.concatenate([s, s[-1:]]).astype(np.float32)
        else:
            sigmas = np.interp(ts, np.arange(0, len(sigmas)), sigmas)
            sigma_last = ((1 - self.alphas_cumprod[0]) / self.alphas_cumprod[0]) ** 0.5
            sigmas = np.concatenate([sigmas, [sigma_last]]).astype(np.float32)
        self.sigmas, self.timesteps = sigmas, ts.astype(np.int64)
        self.num_inference_steps = len(ts)
        self.model_outputs = [None] * c.solver_order
        self.lower_order_nums = 0
        self._step_index = None

    def scale_model_input(self, sample, *args, **kwargs):
        return sample

    @staticmethod
    def _sigma_to_alpha_sigma_t(sigma):
        alpha_t = 1 / ((sigma ** 2 + 1) ** 0.5)
        return alpha_t, sigma * alpha_t

    def convert_model_output(self, model_output, sample):
        """model output -> x0 prediction (dpmsolver++) or epsilon prediction (dpmsolver), :407-506"""
        a, s = (float(v) for v in self._sigma_to_alpha_sigma_t(self.sigmas[self._step_index]))
        pt = self.config.prediction_type
        if pt not in ("epsilon", "sample", "v_prediction"):
            raise ValueError(f"prediction_type given as {pt} must be one of `epsilon`, `sample`, or `v_prediction` for the "
                             "DPMSolverMultistepScheduler.")
        if self.config.algorithm_type == "dpmsolver++":
            return (sample - s * model_output) / a if pt == "epsilon" else model_output if pt == "sample" else a * sample - s * model_output
        return model_output if pt == "epsilon" else (sample - a * model_output) / s if pt == "sample" else a * model_output + s * sample

    def _init_step_index(self, timestep):
        c = np.nonzero(self.timesteps == int(timestep))[0]
        self._step_index = len(self.timesteps) - 1 if len(c) == 0 else int(c[1] if len(c) > 1 else c[0])

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self._step_index is None:
            self._init_step_index(timestep)
        c, n, i = self.config, len(self.timesteps), self._step_index
        lower_order_final = i == n - 1 and (c.euler_at_final or (c.lower_order_final and n < 15))
        lower_order_second = i == n - 2 and c.lower_order_final and n < 15
        m = self.convert_model_output(model_output, sample)
        self.model_outputs = self.model_outputs[1:] + [m]
        at, st = self._sigma_to_alpha_sigma_t(self.sigmas[i + 1])
        a0, s0 = self._sigma_to_alpha_sigma_t(self.sigmas[i])
        lt, l0 = np.log(at) - np.log(st), np.log(a0) - np.log(s0)
        h = lt - l0
        pp = c.algorithm_type == "dpmsolver++"
        f = float
        if c.solver_order == 1 or self.lower_order_nums < 1 or lower_order_final:    # first-order update (:508-575)
            prev = (f(st / s0) * sample - f(at * (np.exp(-h) - 1.0)) * m) if pp else (f(at / a0) * sample - f(st * (np.exp(h) - 1.0)) * m)
        else:                                                                          # second-order multistep (:577-698)
            a1, s1 = self._sigma_to_alpha_sigma_t(self.sigmas[i - 1])
            h_0 = l0 - (np.log(a1) - np.log(s1))
            with np.errstate(divide="ignore"):   # Karras schedules repeat the last sigma: h = 0 -> 1 / r0 = 0, like the reference
                r_inv = f(1.0 / (h_0 / h))
            d0, d1 = self.model_outputs[-1], r_inv * (self.model_outputs[-1] - self.model_outputs[-2])
            if pp:
                prev = f(st / s0) * sample - f(at * (np.exp(-h) - 1.0)) * d0
                prev = prev - f(0.5 * at * (np.exp(-h) - 1.0)) * d1 if c.solver_type == "midpoint" else \
                    prev + f(at * ((np.exp(-h) - 1.0) / h + 1.0)) * d1
            else:
                prev = f(at / a0) * sample - f(st * (np.exp(h) - 1.0)) * d0
                prev = prev - f(0.5 * st * (np.exp(h) - 1.0)) * d1 if c.solver_type == "midpoint" else \
                    prev - f(st * ((np.exp(h) - 1.0) / h - 1.0)) * d1
        _ = lower_order_second   # (with solver_order <= 2 the second-order branch is taken whenever history exists)
        if self.lower_order_nums < c.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1
        return _out(prev, return_dict)

    def multistep_coefficients(self, timestep) -> Tuple[float, float, float, float, float]:
        """(p, q, A, B, D) of this step's update as a linear map of the sample x, the model output e and the previous step's
        converted output m1:  m0 = p x + q e  (``convert_model_output``),  prev = A x + B m0 + D (m0 - m1) ; D = 0 on a first-order
        step. Advances ``_step_index`` and ``lower_order_nums`` as ``step`` does. Every schedule value (alpha_t, sigma_t, lambda, h and
        the coefficient expressions) is the float32 numpy expression of ``step`` / ``convert_model_output``, so both see the same
        numbers; the five are composed from them in float64. NotImplementedError when one of them is not finite (heun's 0 / 0 on
        a Karras schedule's repeated last sigma, where ``step`` itself yields NaN)."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self._step_index is None:
            self._init_step_index(timestep)
        c, n, i = self.config, len(self.timesteps), self._step_index
        lower_order_final = i == n - 1 and (c.euler_at_final or (c.lower_order_final and n < 15))
        a, s = (float(v) for v in self._sigma_to_alpha_sigma_t(self.sigmas[i]))
        pt, pp, f = c.prediction_type, c.algorithm_type == "dpmsolver++", float
        if pt not in ("epsilon", "sample", "v_prediction"):
            raise NotImplementedError(f"prediction_type {pt}")
        if pp:
            p, q = (1.0 / a, -s / a) if pt == "epsilon" else (0.0, 1.0) if pt == "sample" else (a, -s)
        else:
            p, q = (0.0, 1.0) if pt == "epsilon" else (1.0 / s, -a / s) if pt == "sample" else (s, a)
        at, st = self._sigma_to_alpha_sigma_t(self.sigmas[i + 1])
        a0, s0 = self._sigma_to_alpha_sigma_t(self.sigmas[i])
        lt, l0 = np.log(at) - np.log(st), np.log(a0) - np.log(s0)
        h = lt - l0
        A, B = (f(st / s0), -f(at * (np.exp(-h) - 1.0))) if pp else (f(at / a0), -f(st * (np.exp(h) - 1.0)))
        D = 0.0
        if not (c.solver_order == 1 or self.lower_order_nums < 1 or lower_order_final):
            a1, s1 = self._sigma_to_alpha_sigma_t(self.sigmas[i - 1])
            h_0 = l0 - (np.log(a1) - np.log(s1))
            with np.errstate(divide="ignore", invalid="ignore"):
                r_inv = f(1.0 / (h_0 / h))
                if c.solver_type == "midpoint":
                    D = -f(0.5 * at * (np.exp(-h) - 1.0)) * r_inv if pp else -f(0.5 * st * (np.exp(h) - 1.0)) * r_inv
                else:
                    D = f(at * ((np.exp(-h) - 1.0) / h + 1.0)) * r_inv if pp else -f(st * ((np.exp(h) - 1.0) / h - 1.0)) * r_inv
        if self.lower_order_nums < c.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1
        if not all(np.isfinite(v) for v in (p, q, A, B, D)):
            raise NotImplementedError("a multistep coefficient of this step is not finite")
        return p, q, A, B, D

    def add_noise(self, original_samples, noise, timesteps):
        a = torch.as_tensor(self.alphas_cumprod)[timesteps].to(original_samples.device)
        while a.dim() < original_samples.dim():
            a = a.unsqueeze(-1)
        return a ** 0.5 * original_samples + (1 - a) ** 0.5 * noise

    def __len__(self):
        return self.config.num_train_timesteps


class UniPCMultistepScheduler:
    """UniPC (scheduling_unipc_multistep.py:31-846): a B(h) predictor of order 1-3 (``multistep_uni_p_bh_update``) whose output the
    next step corrects with the model output it was evaluated at (``multistep_uni_c_bh_update``), usable at 8-15 steps. Implemented:
    ``solver_order`` 1-3, "bh1" / "bh2" ("midpoint" / "heun" / "logrho" become "bh2"), ``predict_x0``, epsilon / sample / v_prediction,
    ``lower_order_final``, ``disable_corrector``, Karras sigmas, the three spacings. Not implemented (NotImplementedError):
    thresholding, ``solver_p``, ``trained_betas``.
    Both halves are linear in the tensors with scalars of the schedule alone: ``unipc_coefficients`` returns them as one row for the
    library's ``mi355x_sd_unipc_update``."""
    order = 1

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
        self.config = SimpleNamespace(**{k: v for k, v in locals().items() if k != "self"})
        if thresholding or solver_p is not None or trained_betas is not None or solver_order not in (1, 2, 3):
            raise NotImplementedError("UniPCMultistepScheduler(mi355x): thresholding, solver_p, trained_betas and solver_order "
                                      "outside 1-3 are not implemented")
        betas = _make_betas(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.alphas_cumprod = np.cumprod(1.0 - betas, dtype=np.float32)
        self.init_noise_sigma = 1.0
        self.predict_x0, self.disable_corrector, self.solver_p = predict_x0, disable_corrector, None
        self.num_inference_steps = None
        self.timesteps = np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=np.float32)[::-1].copy().astype(np.int64)
        self.model_outputs = [None] * solver_order
        self.timestep_list = [None] * solver_order
        self.lower_order_nums = 0
        self.last_sample = None
        self.this_order = None
        self._step_index = None

    @property
    def step_index(self):
        return self._step_index

    coefficient_walk = _coefficient_walk("_step_index", "lower_order_nums", "model_outputs", "timestep_list", "last_sample",
                                         "this_order")   # (unipc_coefficients)

    def set_timesteps(self, num_inference_steps: int):
        c, n, T = self.config, num_inference_steps, self.config.num_train_timesteps
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif c.timestep_spacing == "leading":
            ts = (np.arange(0, n + 1) * (T // (n + 1))).round()[::-1][:-1].copy().astype(np.int64) + c.steps_offset
        elif c.timestep_spacing == "trailing":
            ts = np.arange(T, 0, -T / n).round().copy().astype(np.int64) - 1
        else:
            raise ValueError(f"{c.timestep_spacing} is not supported. Please make sure to choose one of 'linspace', "
                             "'leading' or 'trailing'.")
        sigmas = np.array(((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5)
        if c.use_karras_sigmas:
            log_sigmas = np.log(sigmas)
            s = np.flip(sigmas).copy()
            rho, ramp = 7.0, np.linspace(0, 1, n)
            lo, hi = s[-1].item() ** (1 / rho), s[0].item() ** (1 / rho)
            s = (hi + ramp * (lo - hi)) ** rho
            ts = np.array([EulerDiscreteScheduler._sigma_to_t(x, log_sigmas) for x in s]).round()
            sigmas = np.concatenate([s, s[-1:]]).astype(np.float32)
        else:
            sigmas = np.interp(ts, np.arange(0, len(sigmas)), sigmas)
            sigma_last = ((1 - self.alphas_cumprod[0]) / self.alphas_cumprod[0]) ** 0.5
            sigmas = np.concatenate([sigmas, [sigma_last]]).astype(np.float32)
        self.sigmas, self.timesteps = sigmas, ts.astype(np.int64)
        self.num_inference_steps = len(ts)
        self.model_outputs = [None] * c.solver_order
        self.lower_order_nums = 0
        self.last_sample = None
        self._step_index = None

    def scale_model_input(self, sample, *args, **kwargs):
        return sample

    _sigma_to_alpha_sigma_t = staticmethod(DPMSolverMultistepScheduler._sigma_to_alpha_sigma_t)

    def _convert_pq(self):
        """(p, q) with convert_model_output = p * sample + q * model_output, from this step's float32 alpha_t and sigma_t"""
        a, s = (float(v) for v in self._sigma_to_alpha_sigma_t(self.sigmas[self._step_index]))
        pt = self.config.prediction_type
        if pt not in ("epsilon", "sample", "v_prediction"):
            raise ValueError(f"prediction_type given as {pt} must be one of `epsilon`, `sample`, or `v_prediction` for the "
                             "UniPCMultistepScheduler.")
        if self.predict_x0:
            return (1.0 / a, -s / a) if pt == "epsilon" else (0.0, 1.0) if pt == "sample" else (a, -s)
        return (0.0, 1.0) if pt == "epsilon" else (1.0 / s, -a / s) if pt == "sample" else (s, a)

    def convert_model_output(self, model_output, *args, sample=None, **kwargs):
        """model output -> x0 prediction (predict_x0) or epsilon prediction, :368-436"""
        if sample is None:
            if len(args) < 2:
                raise ValueError("missing `sample` as a required keyward argument")
            sample = args[1]
        a, s = (float(v) for v in self._sigma_to_alpha_sigma_t(self.sigmas[self._step_index]))
        pt = self.config.prediction_type
        self._convert_pq()   # (the prediction_type check)
        if self.predict_x0:
            return (sample - s * model_output) / a if pt == "epsilon" else model_output if pt == "sample" else a * sample - s * model_output
        return model_output if pt == "epsilon" else (sample - a * model_output) / s if pt == "sample" else a * model_output + s * sample

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

    def _init_step_index(self, timestep):
        c = np.nonzero(self.timesteps == int(timestep))[0]
        # "the sigma index that is taken for the **very** first `step` is always the second index": an img2img start on a
        # duplicated timestep must not skip a sigma
        self._step_index = len(self.timesteps) - 1 if len(c) == 0 else int(c[1] if len(c) > 1 else c[0])

    def _use_corrector(self):
        return self._step_index > 0 and self._step_index - 1 not in self.disable_corrector and self.last_sample is not None

    def _next_order(self):
        c = self.config
        this_order = min(c.solver_order, len(self.timesteps) - self._step_index) if c.lower_order_final else c.solver_order
        return min(this_order, self.lower_order_nums + 1)   # warm-up of the multistep history

    def step(self, model_output, timestep, sample, return_dict: bool = True):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
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
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self._step_index is None:
            self._init_step_index(timestep)
        i, f = self._step_index, float
        p, q = self._convert_pq()
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
        if not all(np.isfinite(v) for v in row):
            raise NotImplementedError("a UniPC coefficient of this step is not finite")
        return tuple(row)

    def add_noise(self, original_samples, noise, timesteps):
        """:822-843: alpha_t x + sigma_t noise with the sigma of each timestep's index in the CURRENT schedule"""
        ts = np.atleast_1d(np.asarray(timesteps.detach().cpu() if torch.is_tensor(timesteps) else timesteps)).astype(np.int64)
        idx = [int(np.nonzero(self.timesteps == t)[0].item()) for t in ts]
        alpha_t, sigma_t = self._sigma_to_alpha_sigma_t(np.asarray(self.sigmas, dtype=np.float32)[idx])
        alpha_t = torch.as_tensor(alpha_t).to(original_samples.device, original_samples.dtype)
        sigma_t = torch.as_tensor(sigma_t).to(original_samples.device, original_samples.dtype)
        while alpha_t.dim() < original_samples.dim():
            alpha_t, sigma_t = alpha_t.unsqueeze(-1), sigma_t.unsqueeze(-1)
        return alpha_t * original_samples + sigma_t * noise

    def __len__(self):
        return self.config.num_train_timesteps


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


class LCMScheduler:
    """Multistep consistency sampling for latent-consistency models / LCM-LoRA (scheduling_lcm.py:140-631): the schedule is a
    subset of the ``original_inference_steps`` distillation schedule, each step predicts x0, applies the boundary-condition
    scalings (c_skip, c_out) and -- except on the last step -- re-noises to the next timestep with fresh noise."""
    order = 1

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", original_inference_steps: int = 50, clip_sample: bool = False,
                 clip_sample_range: float = 1.0, set_alpha_to_one: bool = True, steps_offset: int = 0,
                 prediction_type: str = "epsilon", timestep_spacing: str = "leading", timestep_scaling: float = 10.0):
        self.config = SimpleNamespace(**{k: v for k, v in locals().items() if k != "self"})
        betas = _make_betas(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.alphas_cumprod = np.cumprod(1.0 - betas, dtype=np.float32)
        self.final_alpha_cumprod = np.float32(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64)
        self.custom_timesteps = False
        self._step_index: Optional[int] = None

    @property
    def step_index(self):
        return self._step_index

    def scale_model_input(self, sample, timestep=None):
        return sample

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
        self._step_index = None

    def _init_step_index(self, timestep):
        idx = np.nonzero(self.timesteps == int(timestep))[0]
        self._step_index = int(idx[1] if len(idx) > 1 else idx[0])

    def get_scalings_for_boundary_condition_discrete(self, timestep):
        sigma_data = 0.5
        st = float(timestep) * self.config.timestep_scaling
        return sigma_data ** 2 / (st ** 2 + sigma_data ** 2), st / (st ** 2 + sigma_data ** 2) ** 0.5

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True, *, noise=None):
        """-> prev_sample (and ``denoised``, the x0 estimate the LCM pipeline decodes). ``noise`` (extension): the re-noising
        draw, otherwise ``torch.randn`` from ``generator``."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating "
                             "the scheduler")
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

    def add_noise(self, original_samples, noise, timesteps):
        a = torch.as_tensor(self.alphas_cumprod)[torch.as_tensor(timesteps).long().cpu()].to(original_samples.device)
        while a.dim() < original_samples.dim():
            a = a.unsqueeze(-1)
        return a ** 0.5 * original_samples + (1 - a) ** 0.5 * noise

    def __len__(self):
        return self.config.num_train_timesteps
