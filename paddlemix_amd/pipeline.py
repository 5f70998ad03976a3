"""The denoising loop of ``StableDiffusionPipeline.__call__`` / ``StableDiffusionXLPipeline.__call__`` with the
MI355X UNet in the ``unet`` slot.

Mirrors ppdiffusers/ppdiffusers/pipelines/stable_diffusion/pipeline_stable_diffusion.py:813-908 (SDXL:
stable_diffusion_xl/pipeline_stable_diffusion_xl.py:1039-1093): classifier-free-guidance batch doubling,
``scheduler.scale_model_input``, the UNet call, the guidance combine (+ optional ``rescale_noise_cfg`` :69-80),
``scheduler.step`` and ``callback_on_step_end``, then -- when a ``vae`` is given and ``output_type`` is not "latent" --
``vae.decode(latents / scaling_factor)`` and the image processor's denormalise (:911-925,
image_processor.py VaeImageProcessor.postprocess).  Prompt encoding (CLIP / T5) is a "next row" of SURVEY.md 8f and
stays outside: the loop starts from ``prompt_embeds``.
"""
from __future__ import annotations

import inspect
import warnings
from contextlib import nullcontext
from typing import Callable, Dict, Optional

import numpy as np
import torch

from . import _lib, panorama_forms, program, sega_forms
from .step_forms import FORMS


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale=0.0):
    dims = list(range(1, noise_pred_text.ndim))
    std_text = noise_pred_text.std(dim=dims, keepdim=True)
    std_cfg = noise_cfg.std(dim=dims, keepdim=True)
    rescaled = noise_cfg * (std_text / std_cfg)
    return guidance_rescale * rescaled + (1 - guidance_rescale) * noise_cfg


class _GenericTail:
    """A step of StableDiffusionDenoiser around the UNet: ``scale`` its input for step i, ``update`` the latents from its output (with
    the call's guidance scale, and its guidance rescale or 0.0). Here: the scheduler's own methods, the guidance combine in torch."""

    def __init__(self, scheduler, extra):
        self.scheduler, self.extra = scheduler, extra

    def scale(self, x, i, t):
        return self.scheduler.scale_model_input(x, t)

    def update(self, latents, noise_pred, i, t, do_cfg, guidance_scale, guidance_rescale):
        if do_cfg:
            noise_uncond, noise_text = noise_pred.chunk(2)
            noise_pred = noise_uncond + guidance_scale * (noise_text - noise_uncond)
            if guidance_rescale > 0.0:
                noise_pred = rescale_noise_cfg(noise_pred, noise_text, guidance_rescale)
        return self.scheduler.step(noise_pred, t, latents, return_dict=False, **self.extra)[0]


class _FusedTail:
    """Guidance combine (+ rescale) and scheduler update as ONE device pass over the latents on the caller's stream, coefficients in a
    device table. Not through paddlemix_amd.ops: its wrappers refuse the emulator's host tensors and validate every call.
    A subclass is one row of _TAILS and names its ``form``, a row of step_forms.FORMS: the scheduler method whose rows it runs, the
    library entry it needs with its operands, the state it owns and the noise it draws."""

    form = None              # the row; the four below are read from it
    walk = None              # the scheduler method that gives a step's coefficient row
    whole_schedule = False   # a row depends on the steps before it: the walk covers the timesteps the loop RUNS. True: a stateless
    #                          row, walked over the scheduler's WHOLE schedule together with its model_input_scale
    entry = None             # the library entry every step needs (a test backend from before it keeps the generic path)
    rescale_entry = None     # ... and the one it needs instead under the guidance rescale

    def __init_subclass__(cls):
        """what the row alone decides, once per class: the attributes above and where each operand sits in the call"""
        form, at = cls.form, {k: n for n, k in enumerate(cls.form.operands)}
        cls.symbol = "mi355x_sd_" + form.entry
        cls.walk, cls.whole_schedule = form.walk, form.whole_schedule
        cls.entry, cls.rescale_entry = (None, cls.symbol) if form.always_rescale else (cls.symbol, None)
        cls.stride = 4 * form.width   # bytes of a row
        cls.at_out, cls.at_coef, cls.at_noise, cls.at_order = at["out"], at["coef"], at.get("noise"), at.get("order")
        cls.owned = [(k, at[k], planes) for k, planes in form.state.items()]
        # a written operand the tail owns through the read one it may be itself (multistep: m_out is m_prev's plane)
        cls.shared = [(at[w], at[r]) for w, r in form.same if r in form.state]
        cls.blank = [None] * (len(at) + 5)   # the operands, then guidance_scale, guidance_rescale, batch, per_sample, stream

    def __init__(self, lib, emulated, coef, scales, scheduler, generator):
        self.lib, self.emulated, self.coef, self.scales, self.generator = lib, emulated, coef, scales, generator
        self.order = None if self.at_order is None else scheduler.config.solver_order
        self.noisy = self.form.noise == "fresh" or \
            (self.form.noise == "reused" and "generator" in inspect.signature(scheduler.step).parameters)
        self.noise = self.args = None

    def scale(self, x, i, t):
        return x if self.scales is None else x * self.scales[i]

    def update(self, latents, noise_pred, i, t, do_cfg, guidance_scale, guidance_rescale):
        if self.noisy:   # the ``torch.randn`` call of the scheduler's ``step``, from the call's generator: one seed, the same noise
            self.noise = torch.randn(latents.shape, generator=self.generator, device=latents.device, dtype=torch.float32,
                                     out=self.noise if self.form.noise == "reused" else None)
        lat = latents.contiguous()
        out = torch.empty_like(lat)
        eps = noise_pred.data_ptr()
        _lib.check(self.launch(lat, eps, eps + 4 * lat.numel() if do_cfg else None, out, i, float(guidance_scale),
                               float(guidance_rescale), program.caller_stream(self.coef.device, self.emulated)))
        return out

    def _first(self, lat, i):
        """What no step changes, on the first one: the entry, the state the tail owns (never initialised: the first row reads none of
        it), the address of row 0 and the call's arguments in the row's operand order with the state's pointers, ``order``, batch and
        per_sample in place -- a step fills in the rest"""
        a, self.state = list(self.blank), {}
        for k, at, planes in self.owned:
            t = self.state[k] = torch.empty_like(lat) if planes == 1 else lat.new_empty((planes or self.order,) + tuple(lat.shape))
            a[at] = t.data_ptr()
        for w, r in self.shared:
            a[w] = a[r]
        if self.order:
            a[self.at_order] = self.order
        a[-3], a[-2] = lat.shape[0], lat.numel() // lat.shape[0]
        self.row0 = self.coef.data_ptr() - (0 if self.whole_schedule else self.stride * i)
        self.fn, self.args = getattr(self.lib, self.symbol), a

    def launch(self, lat, eps, eps_text, out, i, gs, gr, stream):
        if self.args is None:
            self._first(lat, i)
        a = self.args
        a[0], a[1], a[2] = lat.data_ptr(), eps, eps_text   # (every form starts with x, eps_uncond, eps_text)
        a[self.at_out], a[self.at_coef] = out.data_ptr(), self.row0 + self.stride * i
        if self.noisy:
            a[self.at_noise] = self.noise.data_ptr()
        a[-5], a[-4], a[-1] = gs, gr, stream
        return self.fn(*a)


class _LinearTail(_FusedTail):
    """``step_coefficients`` (DDIM at eta = 0, Euler; epsilon and v prediction): prev = a * x + b * model_output, (a, b) = row i of a
    table [steps, 2] over the scheduler's WHOLE schedule; ``scales``: that schedule's model-input scales"""

    form = FORMS["guidance"]

    def launch(self, lat, eps, eps_text, out, i, gs, gr, stream):
        n, cp = lat.numel(), self.coef.data_ptr() + self.stride * i
        if gr > 0.0:
            return self.lib.mi355x_sd_cfg_rescale_axpby(lat.data_ptr(), eps, eps_text, out.data_ptr(), cp, gs, gr, lat.shape[0],
                                                        n // lat.shape[0], stream)
        if eps_text is not None:
            return self.lib.mi355x_sd_cfg_axpby(lat.data_ptr(), eps, eps_text, out.data_ptr(), cp, gs, n, stream)
        return self.lib.mi355x_sd_axpby(lat.data_ptr(), eps, out.data_ptr(), cp, n, stream)


class _MultistepTail(_FusedTail):
    """``multistep_coefficients`` (DPM-Solver multistep): convert_model_output and the history shuffle ride in the same launch;
    (p, q, A, B, D) = row i - first of a table [steps, 5] over the steps the loop RUNS (img2img starts inside the schedule)"""

    form = FORMS["multistep"]


class _UniPCTail(_FusedTail):
    """``unipc_coefficients`` (UniPC): convert_model_output, the corrector, the predictor, last_sample and the history shift ride in
    the same launch; the 12 coefficients = row i - first of a table [steps, 12] over the steps the loop RUNS. The tail owns ``last``
    and the ``order`` planes of ``hist``; the first row forms no term that reads them, so fresh ones are not initialised"""

    form = FORMS["unipc"]


class _AncestralTail(_FusedTail):
    """``ancestral_coefficients`` (Euler a): prev = a * x + b * model_output + c * z, (a, b, c) = row i of a table [steps, 3] over the
    scheduler's WHOLE schedule, ``scales`` as in _LinearTail. z is drawn here, once per step, by the ``torch.randn`` call of the
    scheduler's ``step`` from the call's generator -- one seed gives the same noise on both paths -- and the launch reads it; the last
    row has c = 0 and its plane is drawn (the generator advances as in ``step``) but not read"""

    form = FORMS["ancestral"]


class _HeunTail(_FusedTail):
    """``heun_coefficients`` (Heun): one launch per model evaluation, 2n - 1 for n steps; (p, q, h, g, second) = row i of a table
    [2n - 1, 5] over the scheduler's WHOLE schedule (even rows: stage 1, odd rows: stage 2), ``scales`` as in _LinearTail. The tail
    owns the step's parked sample and derivative; stage 1 writes them without reading, so fresh ones are not initialised, and their
    pointers stay fixed for the whole loop"""

    form = FORMS["heun"]


class _Dpm2Tail(_FusedTail):
    """``dpm2_coefficients`` (DPM2, DPM2 a): one launch per model evaluation, 2n - 1 for n steps; (p, q, h, c, second) = row i of a
    table [2n - 1, 5] over the scheduler's WHOLE schedule (even rows: stage 1, odd rows: stage 2), ``scales`` as in _LinearTail. The
    tail owns the step's parked sample; stage 1 writes it without reading, so a fresh one is not initialised, and its pointer stays
    fixed for the whole loop. For the ancestral class (its ``step`` takes a generator) z is drawn here, once per evaluation, by the
    ``torch.randn`` call of that ``step`` from the call's generator -- one seed gives the same noise on both paths; after the first
    evaluation the draw goes into the same buffer (``out=``: the same values, the same generator state), so the noise pointer stays
    fixed too. Only the stage-2 rows read the plane. DPM2 draws nothing and passes a null noise (c = 0 on every row)"""

    form = FORMS["dpm2"]


class _PlmsTail(_FusedTail):
    """``plms_coefficients`` (PNDM with ``skip_prk_steps``: PLMS): one launch per model evaluation, n + 1 for n steps; the 12 values =
    row i - first of a table [evaluations, 12] over the timesteps the loop RUNS (the kind of evaluation depends on how many this loop
    has made, not on its place in the schedule). The tail owns the parked sample and the ring of three model outputs; the first row
    reads neither and every later one only what an earlier launch wrote, so fresh ones are not initialised, no plane is ever copied
    and their pointers stay fixed for the whole loop"""

    form = FORMS["plms"]


class _SinglestepTail(_FusedTail):
    """``singlestep_coefficients`` (DPM-Solver singlestep): one launch per model evaluation; (p, q, A, B, E1, E2, order, keep) = row
    i - first of a table [evaluations, 8] over the timesteps the loop RUNS (an img2img loop starts inside the schedule, where the
    listed order may not be possible yet). The tail owns the parked sample and the two planes of the group's converted outputs; the
    first row has order 1 and reads neither, every later one reads only what an earlier launch of its group wrote, so fresh ones are
    not initialised, no plane is ever copied and their pointers stay fixed for the whole loop"""

    form = FORMS["singlestep"]


# in priority order: the first whose walk the scheduler has
_TAILS = (_UniPCTail, _MultistepTail, _AncestralTail, _HeunTail, _Dpm2Tail, _PlmsTail, _SinglestepTail, _LinearTail)


class _VaeSwitches:
    """``enable_vae_tiling`` / ``enable_vae_slicing`` of the reference's pipelines (pipeline_stable_diffusion.py enable_vae_slicing /
    enable_vae_tiling and their disable_ twins): forwarded to the ``vae`` the pipeline owns."""

    def _vae(self):
        if self.vae is None:
            raise ValueError("this pipeline was built without a `vae`")
        return self.vae

    def _postprocess(self, output_type: str, decode):
        """VaeImageProcessor.postprocess of ``decode()``, the denoiser's own way of putting its latents through the VAE"""
        if self.vae is None:
            raise ValueError("output_type != 'latent' needs a `vae`")
        if output_type not in ("pt", "np"):
            raise ValueError(f"output_type must be 'latent', 'pt' or 'np', got {output_type!r}")
        image = (decode() / 2 + 0.5).clamp(0, 1)
        return image if output_type == "pt" else image.cpu().permute(0, 2, 3, 1).float().numpy()

    def enable_vae_slicing(self) -> None:
        self._vae().enable_slicing()

    def disable_vae_slicing(self) -> None:
        self._vae().disable_slicing()

    def enable_vae_tiling(self) -> None:
        self._vae().enable_tiling()

    def disable_vae_tiling(self) -> None:
        self._vae().disable_tiling()


class StableDiffusionDenoiser(_VaeSwitches):
    """``pipe = StableDiffusionDenoiser(unet, scheduler); latents = pipe(prompt_embeds=..., ...)``"""

    def __init__(self, unet, scheduler, vae=None, text_encoder=None, text_encoder_2=None, controlnet=None, adapter=None):
        self.unet, self.scheduler, self.vae = unet, scheduler, vae
        self.text_encoder, self.text_encoder_2 = text_encoder, text_encoder_2
        self.controlnet = controlnet   # ControlNetModel: StableDiffusionControlNetPipeline (controlnet/pipeline_controlnet.py)
        self.adapter = adapter         # T2IAdapter / MultiAdapter: StableDiffusion(XL)AdapterPipeline (pipelines/t2i_adapter/)

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float) -> None:
        """FreeU on the U-Net's first two up blocks (pipeline_stable_diffusion.py ``enable_freeu`` -> ``unet.enable_freeu``); holds
        with every scheduler tail and with a ControlNet, whose own model has no up path and is left alone"""
        self.unet.enable_freeu(s1=s1, s2=s2, b1=b1, b2=b2)

    def disable_freeu(self) -> None:
        self.unet.disable_freeu()

    def encode_prompt(self, input_ids: torch.Tensor, input_ids_2: Optional[torch.Tensor] = None,
                      clip_skip: Optional[int] = None):
        """Token ids -> (prompt_embeds, pooled_prompt_embeds or None). Tokenisation stays with the caller (the CLIP
        vocabulary files are not part of a model's weights).
        SD (one encoder, pipeline_stable_diffusion.py:368-391): ``text_encoder(ids)[0]``.
        SDXL (two encoders, pipeline_stable_diffusion_xl.py:363-375): hidden_states[-2] of both encoders concatenated on
        the channel axis, pooled = ``text_encoder_2(ids)[0]`` (the projected EOS row)."""
        if self.text_encoder is None:
            raise ValueError("encode_prompt needs a `text_encoder`")
        if self.text_encoder_2 is None:
            if clip_skip is None:
                return self.text_encoder(input_ids)[0], None
            # :378-391: the hidden state clip_skip layers before the last, then the encoder's final LayerNorm
            hidden = self.text_encoder(input_ids, output_hidden_states=True).hidden_states[-(clip_skip + 1)]
            return self.text_encoder.text_model.final_layer_norm(hidden), None
        embeds, pooled = [], None
        for enc, ids in ((self.text_encoder, input_ids), (self.text_encoder_2, input_ids if input_ids_2 is None else input_ids_2)):
            out = enc(ids, output_hidden_states=True)
            pooled = out[0]   # only the final encoder's pooled output is kept
            embeds.append(out.hidden_states[-2 if clip_skip is None else -(clip_skip + 2)])
        return torch.cat(embeds, dim=-1), pooled

    def get_add_time_ids(self, original_size, crops_coords_top_left, target_size, text_encoder_projection_dim: int,
                         device=None) -> torch.Tensor:
        """pipeline_stable_diffusion_xl.py:603-619"""
        ids = list(original_size + crops_coords_top_left + target_size)
        cfg = self.unet.config
        passed = cfg.addition_time_embed_dim * len(ids) + text_encoder_projection_dim
        if passed != cfg.projection_class_embeddings_input_dim:
            raise ValueError(f"Model expects an added time embedding vector of length "
                             f"{cfg.projection_class_embeddings_input_dim}, but a vector of {passed} was created.")
        return torch.tensor([ids], dtype=torch.float32, device=device)

    def _fused_plan(self, rescale: bool, device, timesteps=None, generator=None):
        """The fused step tail, when the scheduler's step is an update the library runs in one launch; None -> the generic path.
        The library always has every entry (its ABI version is checked at load); a test backend from before one keeps that path."""
        sch = self.scheduler
        lib, emulated = getattr(self.unet, "_lib", None), getattr(self.unet, "_emulated", False)
        tail = next((c for c in _TAILS if hasattr(sch, c.walk)), None)
        entry = tail and ((rescale and tail.rescale_entry) or tail.entry)
        if lib is None or tail is None or (emulated and entry and not hasattr(lib, entry)):
            return None
        scales, coefs, walk = [] if tail.whole_schedule else None, [], getattr(sch, tail.walk)
        try:
            with getattr(sch, "coefficient_walk", nullcontext)():   # the walk advances the scheduler's step state: put back on exit
                for t in (sch.timesteps if tail.whole_schedule else timesteps):
                    if tail.whole_schedule:
                        scales.append(float(sch.model_input_scale(t)) if hasattr(sch, "model_input_scale") else 1.0)
                    coefs.append(tuple(float(v) for v in walk(t)))
        except NotImplementedError:
            return None
        coef = torch.tensor(coefs, dtype=torch.float32, device=device).contiguous()
        return tail(lib, emulated, coef, scales, sch, generator)

    def _adapter_state(self, adapter_image, hw, scale, batch: int, do_cfg: bool):
        """The adapter's features for the whole loop (pipeline_stable_diffusion_adapter.py:757-766, 823-836): the image(s) cropped to
        the multiple of the downscale factor the call runs at, one adapter forward, the conditioning scale, the prompt batch, the
        doubling under classifier-free guidance"""
        from .adapter import MultiAdapter
        crop = lambda im: im[..., :hw[0], :hw[1]].to(torch.float32).contiguous()  # noqa: E731
        if isinstance(self.adapter, MultiAdapter):
            if torch.is_tensor(adapter_image):
                raise ValueError("a MultiAdapter takes a list of `adapter_image`s, one per adapter")
            weights = list(scale) if isinstance(scale, (list, tuple)) else [scale] * len(adapter_image)
            state = self.adapter([crop(im) for im in adapter_image], weights)
        else:
            if not torch.is_tensor(adapter_image):
                raise ValueError("`adapter_image` has to be a [B, C, H, W] tensor (a list is for a MultiAdapter)")
            if isinstance(scale, (list, tuple)):
                raise ValueError("a list of `adapter_conditioning_scale`s is for a MultiAdapter")
            state = [v * float(scale) for v in self.adapter(crop(adapter_image))]
        out = []
        for v in state:
            if batch % v.shape[0]:
                raise ValueError(f"Cannot duplicate `adapter_image` of batch size {v.shape[0]} to {batch} prompts.")
            v = v.repeat(batch // v.shape[0], 1, 1, 1)
            out.append(torch.cat([v] * 2) if do_cfg else v)
        return out

    def decode_latents(self, latents: torch.Tensor, output_type: str = "pt", circular_padding: bool = False):
        """pipeline_stable_diffusion.py:911 + VaeImageProcessor.postprocess: decode, (x / 2 + 0.5).clamp(0, 1).
        ``circular_padding``: ``decode_latents_with_padding`` (pipeline_stable_diffusion_panorama.py:371-382): the last
        panorama_forms.CIRCULAR_PAD latent columns are put in front and the first ones behind, the padded latents go through the same
        decode (tiling included), and the pixels of the padding are cropped from both sides."""
        if circular_padding:
            pad, width = panorama_forms.CIRCULAR_PAD, latents.shape[-1]
            latents = torch.cat((latents[..., -pad:], latents, latents[..., :pad]), dim=-1)

        def decode():
            image = decode_padded()
            if circular_padding:
                px = pad * (image.shape[-1] // (width + 2 * pad))
                image = image[..., px:-px]
            return image

        def decode_padded():
            vc = self.vae.config
            mean, std = getattr(vc, "latents_mean", None), getattr(vc, "latents_std", None)
            if mean is None or std is None:
                return self.vae.decode(latents, return_dict=False, in_scale=1.0 / vc.scaling_factor)[0]
            # StableDiffusionXLPipeline (pipeline_stable_diffusion_xl.py:1105-1110): VAEs that publish per-channel latent statistics
            # are denormalised with them instead of the plain 1 / scaling_factor
            shape = (1, -1, 1, 1)
            z = latents * torch.as_tensor(std, dtype=latents.dtype, device=latents.device).reshape(shape) / vc.scaling_factor \
                + torch.as_tensor(mean, dtype=latents.dtype, device=latents.device).reshape(shape)
            return self.vae.decode(z, return_dict=False)[0]

        return self._postprocess(output_type, decode)

    def prepare_latents(self, batch_size, num_channels_latents, height, width, dtype, generator=None, latents=None,
                        device=None):
        shape = (batch_size, num_channels_latents, height, width)
        if latents is None:
            latents = torch.randn(shape, generator=generator, dtype=dtype, device=device)
        elif tuple(latents.shape) != shape:
            raise ValueError(f"Unexpected latents shape, got {tuple(latents.shape)}, expected {shape}")
        return latents * self.scheduler.init_noise_sigma  # pipeline_stable_diffusion.py:581-586

    @staticmethod
    def get_guidance_scale_embedding(w: torch.Tensor, embedding_dim: int = 512) -> torch.Tensor:
        """sinusoidal embedding of (guidance_scale - 1) for guidance-distilled UNets (LCM; pipeline_stable_diffusion.py:588-616)
        -> fp32 [len(w), embedding_dim], the UNet's ``timestep_cond``"""
        if w.dim() != 1:
            raise ValueError("w: expected a 1-D tensor of guidance scales")
        half = embedding_dim // 2
        freq = torch.exp(torch.arange(half, dtype=torch.float32, device=w.device) * -(np.log(10000.0) / (half - 1)))
        emb = (w.to(torch.float32) * 1000.0)[:, None] * freq[None, :]
        emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=1)
        if embedding_dim % 2 == 1:
            emb = torch.nn.functional.pad(emb, (0, 1))
        return emb

    def _encode_image(self, image: torch.Tensor, generator) -> torch.Tensor:
        """``_encode_vae_image`` (pipeline_stable_diffusion_inpaint.py:746-758): posterior sample * scaling_factor"""
        if self.vae is None:
            raise ValueError("an image input needs a `vae` with encoder parameters")
        return self.vae.encode(image.to(torch.float32)).latent_dist.sample(generator, out_scale=self.vae.config.scaling_factor)

    def prepare_inpaint(self, image, mask_image, masked_image_latents, timesteps, batch_size: int, generator,
                        is_strength_max: bool, do_cfg: bool):
        """``prepare_latents`` + ``prepare_mask_latents`` of the inpaint pipeline (pipeline_stable_diffusion_inpaint.py:689-803),
        in the reference's order of random draws: image posterior, initial noise, masked-image posterior."""
        lc = self.vae.config.latent_channels if self.vae is not None else 4
        four = self.unet.config.in_channels == lc
        if not torch.is_tensor(image) or image.dim() != 4 or not torch.is_tensor(mask_image) or mask_image.dim() != 4:
            raise ValueError("`image` and `mask_image` have to be [B, C, H, W] tensors")
        image = image.to(torch.float32)
        f = 2 ** (len(self.vae.config.block_out_channels) - 1) if self.vae is not None else 8     # vae_scale_factor
        hl, wl = (image.shape[-2], image.shape[-1]) if image.shape[1] == lc else (image.shape[-2] // f, image.shape[-1] // f)
        image_latents = None
        if four or not is_strength_max:
            image_latents = image if image.shape[1] == lc else self._encode_image(image, generator)
            image_latents = image_latents.repeat(batch_size // image_latents.shape[0], 1, 1, 1)
        noise = torch.randn((batch_size, lc, hl, wl), generator=generator, dtype=torch.float32, device=image.device)
        if is_strength_max:
            latents = noise * self.scheduler.init_noise_sigma
        else:
            ts = torch.as_tensor(np.asarray(timesteps[:1]).reshape(-1)).repeat(batch_size)
            latents = self.scheduler.add_noise(image_latents, noise, ts)
        mask_px = (mask_image.to(torch.float32) >= 0.5).to(torch.float32)          # mask_processor: do_binarize
        mask = torch.nn.functional.interpolate(mask_px, size=(hl, wl))              # nearest, like the reference (:766-768)
        if masked_image_latents is None:
            if image.shape[1] == lc:
                raise ValueError("latents passed as `image` need `masked_image_latents`")
            masked_image_latents = self._encode_image(image * (mask_px < 0.5).to(image.dtype), generator)   # (:1134)
        for nm, t in (("masks", mask), ("images", masked_image_latents)):
            if batch_size % t.shape[0]:
                raise ValueError(f"The passed {nm} and the required batch size don't match: {t.shape[0]} vs {batch_size}.")
        mask = mask.repeat(batch_size // mask.shape[0], 1, 1, 1)
        mil = masked_image_latents.to(torch.float32).repeat(batch_size // masked_image_latents.shape[0], 1, 1, 1)
        if not four and lc + mask.shape[1] + mil.shape[1] != self.unet.config.in_channels:
            raise ValueError(f"Incorrect configuration settings! The config of `pipeline.unet` expects "
                             f"{self.unet.config.in_channels} but received `num_channels_latents`: {lc} + `num_channels_mask`: "
                             f"{mask.shape[1]} + `num_channels_masked_image`: {mil.shape[1]}")
        rep2 = (lambda t: torch.cat([t] * 2)) if do_cfg else (lambda t: t)
        return latents, dict(mask=mask, noise=noise, image_latents=image_latents, mask_in=rep2(mask), masked_in=rep2(mil))

    def get_timesteps(self, num_inference_steps: int, strength: float):
        """img2img: keep the last ``int(steps * strength)`` steps (pipeline_stable_diffusion_img2img.py:616-623)."""
        init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
        t_start = max(num_inference_steps - init_timestep, 0)
        order = getattr(self.scheduler, "order", 1)
        return self.scheduler.timesteps[t_start * order:], num_inference_steps - t_start, t_start * order

    def prepare_image_latents(self, image: torch.Tensor, timestep, batch_size: int, generator=None) -> torch.Tensor:
        """img2img ``prepare_latents`` (pipeline_stable_diffusion_img2img.py:625-681): encode (unless `image` already has the
        latent channel count), ``* scaling_factor``, duplicate to the prompt batch, ``scheduler.add_noise`` at the first kept
        timestep. The posterior sample and its scaling are one launch (``latent_dist.sample(out_scale=...)``)."""
        if not torch.is_tensor(image) or image.dim() != 4:
            raise ValueError(f"`image` has to be a [B, C, H, W] tensor but is {type(image)}")
        if image.shape[1] == self.unet.config.in_channels:
            init = image.to(torch.float32)
        else:
            if self.vae is None:
                raise ValueError("an image input needs a `vae` with encoder parameters")
            dist = self.vae.encode(image.to(torch.float32)).latent_dist
            init = dist.sample(generator, out_scale=self.vae.config.scaling_factor)
        if batch_size > init.shape[0]:
            if batch_size % init.shape[0]:
                raise ValueError(f"Cannot duplicate `image` of batch size {init.shape[0]} to {batch_size} text prompts.")
            init = torch.cat([init] * (batch_size // init.shape[0]))
        noise = torch.randn(init.shape, generator=generator, dtype=torch.float32, device=init.device)
        ts = torch.as_tensor(np.asarray(timestep).reshape(-1)[:1]).repeat(init.shape[0])
        return self.scheduler.add_noise(init, noise, ts)

    def prepare_ip2p_image_latents(self, image: torch.Tensor, batch_size: int, do_cfg: bool) -> torch.Tensor:
        """InstructPix2Pix ``prepare_image_latents`` (pipeline_stable_diffusion_instruct_pix2pix.py:706-745): the MODE of the
        posterior, left unscaled (no ``scaling_factor``); latents passed as `image` (4 channels) are taken as they are; duplicated to
        the prompt batch with the reference's deprecation warning, or refused with its ValueError; ``[img, img, zeros]`` under guidance. The SDXL pipeline (pipeline_stable_diffusion_xl_instruct_pix2pix.py:
        513-553) differs only in running a float16 VAE in float32 for the encode (:516-526) -- this VAE always encodes from fp32
        input -- and applies no latent statistics (``latents_mean`` / ``latents_std`` enter only its decode, :948-957)."""
        if not torch.is_tensor(image) or image.dim() != 4:
            raise ValueError(f"`image` has to be of type `torch.Tensor` [B, C, H, W] but is {type(image)}")
        image = image.to(torch.float32)
        if image.shape[1] == 4:
            il = image
        else:
            if self.vae is None:
                raise ValueError("an image input needs a `vae` with encoder parameters")
            il = self.vae.encode(image).latent_dist.mode()
        if batch_size > il.shape[0] and batch_size % il.shape[0] == 0:
            warnings.warn(   # (:724-731: the reference's deprecation message, word for word)
                f"You have passed {batch_size} text prompts (`prompt`), but only {il.shape[0]} initial images (`image`). Initial images "
                "are now duplicating to match the number of text prompts. Note that this behavior is deprecated and will be removed in "
                "a version 1.0.0. Please make sure to update your script to pass as many initial images as text prompts to suppress "
                "this warning.", FutureWarning, stacklevel=2)
            il = torch.cat([il] * (batch_size // il.shape[0]), dim=0)
        elif batch_size > il.shape[0]:
            raise ValueError(f"Cannot duplicate `image` of batch size {il.shape[0]} to {batch_size} text prompts.")
        if do_cfg:
            il = torch.cat([il, il, torch.zeros_like(il)], dim=0)
        return il.contiguous()

    def _instruct_pix2pix(self, prompt_embeds, negative_prompt_embeds, image, num_inference_steps, guidance_scale,
                          image_guidance_scale, guidance_rescale, latents, generator, added_cond_kwargs, negative_added_cond_kwargs,
                          callback_on_step_end, vae_scale_factor, output_type, ids, original_size, crops_coords_top_left, target_size,
                          fused_update, eta):
        """The loop of StableDiffusionInstructPix2PixPipeline.__call__ (pipeline_stable_diffusion_instruct_pix2pix.py:283-430) and of
        its SDXL twin (pipeline_stable_diffusion_xl_instruct_pix2pix.py:756-938). Per step two launches around the U-Net:
        ``mi355x_sd_ip2p_input`` builds ``[scale * latents | image latents]`` for the three guidance groups (:373-377), and
        ``mi355x_sd_guidance3`` writes the guided output (:394-400; with ``guidance_rescale`` also rescale_noise_cfg, SDXL :917-919, on
        the predicted originals when the scheduler has ``sigmas``, :903-906, :927-928). The scheduler's tail then runs with no guidance
        of its own. Without the rescale the reference's detour through predicted originals cancels in real arithmetic -- the three
        weights sum to 1 -- and is not taken."""
        if image is None:
            raise ValueError("`image` input cannot be undefined.")
        if getattr(self.unet.config, "time_cond_proj_dim", None) is not None:
            raise NotImplementedError("a guidance-distilled U-Net (`time_cond_proj_dim`) together with `image_guidance_scale` "
                                      "(InstructPix2Pix) is not implemented")
        lib, emulated = getattr(self.unet, "_lib", None), getattr(self.unet, "_emulated", False)
        if lib is None:
            raise _lib.MI355XError("InstructPix2Pix runs its guidance and input kernels through the U-Net's library: the `unet` has none")
        do_cfg = guidance_scale > 1.0 and image_guidance_scale >= 1.0   # (SD :764)
        prompt_ids, negative_prompt_ids, prompt_ids_2, negative_prompt_ids_2 = ids
        pooled = neg_pooled = None
        if prompt_embeds is None:
            if prompt_ids is None:
                raise ValueError("Provide either `prompt_embeds` or `prompt_ids`")
            prompt_embeds, pooled = self.encode_prompt(prompt_ids, prompt_ids_2)
            if do_cfg and negative_prompt_embeds is None:
                if negative_prompt_ids is not None:
                    negative_prompt_embeds, neg_pooled = self.encode_prompt(negative_prompt_ids, negative_prompt_ids_2)
                elif self.text_encoder_2 is not None:   # SDXL: force_zeros_for_empty_prompt
                    negative_prompt_embeds, neg_pooled = torch.zeros_like(prompt_embeds), torch.zeros_like(pooled)
        if do_cfg and negative_prompt_embeds is None:
            raise ValueError("classifier-free guidance needs `negative_prompt_embeds` (or `negative_prompt_ids`)")
        B, cfg, sch = prompt_embeds.shape[0], self.unet.config, self.scheduler
        # asked before ``set_timesteps``, as the reference asks (SD :307 before :323, SDXL :772 before :801): Euler, Euler a, Heun and
        # DPM2 have ``sigmas`` from ``__init__``; the DPM-Solver classes and UniPC build theirs in ``set_timesteps`` and, freshly built,
        # rescale in eps space (they are alpha-space: x - sigma * e is no predicted original there)
        in_sigma_space = hasattr(sch, "sigmas")
        sch.set_timesteps(num_inference_steps)
        timesteps = sch.timesteps
        il = self.prepare_ip2p_image_latents(image, B, do_cfg).to(prompt_embeds.device)
        h, w = il.shape[-2:]
        c_lat = self.vae.config.latent_channels if self.vae is not None else 4
        latents = self.prepare_latents(B, c_lat, h, w, torch.float32, generator, latents, prompt_embeds.device)
        c_img = il.shape[1]
        if c_lat + c_img != cfg.in_channels:   # (SD :353-360)
            raise ValueError(f"Incorrect configuration settings! The config of `pipeline.unet`: {cfg} expects {cfg.in_channels} but "
                             f"received `num_channels_latents`: {c_lat} + `num_channels_image`: {c_img}  = {c_lat + c_img}. Please "
                             "verify the config of `pipeline.unet` or your `image` input.")
        if pooled is not None and added_cond_kwargs is None:   # SDXL micro-conditioning (SDXL :839-852)
            hw = (h * vae_scale_factor, w * vae_scale_factor)
            tids = self.get_add_time_ids(tuple(original_size or hw), tuple(crops_coords_top_left), tuple(target_size or hw),
                                         pooled.shape[-1], pooled.device).repeat(B, 1)
            added_cond_kwargs = {"text_embeds": pooled, "time_ids": tids}
            if do_cfg:
                negative_added_cond_kwargs = {"text_embeds": neg_pooled, "time_ids": tids}
        if do_cfg:   # [text, negative, negative] (SD :591, SDXL :856-860)
            prompt_embeds = torch.cat([prompt_embeds, negative_prompt_embeds, negative_prompt_embeds])
            if added_cond_kwargs is not None:
                neg = negative_added_cond_kwargs or added_cond_kwargs
                added_cond_kwargs = {k: torch.cat([v, neg[k], neg[k]]) for k, v in added_cond_kwargs.items()}
        step_params = inspect.signature(sch.step).parameters
        extra = {}
        if "eta" in step_params:
            extra["eta"] = eta
        if "generator" in step_params:
            extra["generator"] = generator
        dev = latents.device
        tail = (self._fused_plan(False, dev, timesteps, generator) if fused_update and not eta else None) or _GenericTail(sch, extra)
        fused = isinstance(tail, _FusedTail)
        rescale = float(guidance_rescale) if do_cfg and guidance_rescale > 0.0 else 0.0
        sigmas = None
        if rescale and in_sigma_space:   # the loop's sigmas as a device table, uploaded once: a step passes its row's address
            sigmas = torch.tensor(np.asarray(sch.sigmas, dtype=np.float32), device=dev).contiguous()
        groups, per_sample = (3 if do_cfg else 1), c_lat * h * w
        model_in = torch.empty((groups * B, c_lat + c_img, h, w), dtype=torch.float32, device=dev)
        for i, t in enumerate(timesteps):
            stream = program.caller_stream(dev, emulated)
            lat = latents.contiguous()
            if fused:
                x_in, scale = lat, (1.0 if tail.scales is None else tail.scales[i])
            else:
                x_in, scale = tail.scale(lat, i, t).contiguous(), 1.0
            _lib.check(lib.mi355x_sd_ip2p_input(x_in.data_ptr(), il.data_ptr(), model_in.data_ptr(), float(scale), groups, B, c_lat,
                                                c_img, h * w, stream))
            e = self.unet(model_in, t, encoder_hidden_states=prompt_embeds, added_cond_kwargs=added_cond_kwargs, return_dict=False)[0]
            if do_cfg:
                eps, e = e.contiguous(), torch.empty_like(lat)
                x_ptr = row = None
                if sigmas is not None:
                    # the reference's ``(timesteps == t).nonzero()[0]``: the FIRST match (Heun and DPM2 repeat their timesteps)
                    first = int(np.nonzero(np.asarray(sch.timesteps) == np.asarray(t))[0][0])
                    x_ptr, row = lat.data_ptr(), sigmas.data_ptr() + 4 * first
                _lib.check(lib.mi355x_sd_guidance3(eps.data_ptr(), x_ptr, row, e.data_ptr(), float(guidance_scale),
                                                   float(image_guidance_scale), rescale, B, per_sample, stream))
            latents = tail.update(lat, e.contiguous(), i, t, False, 1.0, 0.0)
            if callback_on_step_end is not None:
                out = callback_on_step_end(self, i, t, {"latents": latents})
                latents = out.pop("latents", latents)
        if output_type == "latent":
            return latents
        return self.decode_latents(latents, output_type)

    @staticmethod
    def semantic_guidance_torch(i, raw, n, momentum, extra, guidance_scale, edit_momentum_scale, edit_mom_beta, per_concept):
        """One step of the reference's semantic guidance (pipeline_semantic_stable_diffusion.py:541-699) in torch ops on the device of
        `raw`, the U-Net output of (2 + n) * B samples -> (noise_pred, momentum'): what ``mi355x_sd_sega_guidance`` replaces
        (``fused_guidance=False``; the cross-check and the measurement's other side). One ``torch.quantile`` per live concept."""
        chunks = raw.chunk(2 + n)
        u, t = chunks[0], chunks[1]
        guidance = guidance_scale * (t - u)
        dec = sega_forms.step_decisions(i, n, **per_concept)
        g, weights = [], []
        for (scale, q, weight, _), e in zip(dec, chunks[2:]):
            if weight is None:   # cooled down (:611-613)
                g.append(torch.zeros_like(u))
                weights.append(0.0)
                continue
            d = (e - u) * float(scale)
            thr = torch.quantile(d.abs().flatten(2), q, dim=2, keepdim=False)
            g.append(torch.where(d.abs() >= thr[:, :, None, None], d, torch.zeros_like(d)))
            weights.append(float(weight))
        w = torch.tensor(weights, dtype=u.dtype, device=u.device)
        w = torch.where(w < 0, torch.zeros_like(w), w)
        warm = [c for c, d in enumerate(dec) if d[3]]
        if 0 < len(warm) < n:   # (:654-677; no nan_to_num here)
            wp = w[warm] / w[warm].sum()
            part = torch.zeros_like(u)
            for k, c in enumerate(warm):
                part = part + wp[k] * g[c]
            guidance = guidance + part
        w = torch.nan_to_num(w)
        edit = torch.zeros_like(u)
        for c in range(n):
            edit = edit + w[c] * g[c]
        edit = edit + edit_momentum_scale * momentum
        momentum = edit_mom_beta * momentum + (1 - edit_mom_beta) * edit
        if len(warm) == n:
            guidance = guidance + edit
        if extra is not None:
            guidance = guidance + extra
        return u + guidance, momentum

    def _semantic_guidance(self, prompt_embeds, negative_prompt_embeds, edit_embeds, num_inference_steps, guidance_scale, latents,
                           generator, callback_on_step_end, vae_scale_factor, output_type, ids, height, width, fused_update, eta,
                           fused_guidance, sem_guidance, per_concept, edit_momentum_scale, edit_mom_beta):
        """The loop of SemanticStableDiffusionPipeline.__call__ (pipeline_semantic_stable_diffusion.py:529-707). Per step ONE U-Net call
        on (2 + n) * B samples -- embeddings ``[negative | text | concept 0 | ... | concept n-1]``, B rows each -- then ONE
        ``mi355x_sd_sega_guidance`` (the guidance, every concept's quantile mask, the warm-up regimes, the momentum and
        ``sem_guidance[i]``), its per-step scalars row i of a device table built once (sega_forms.rows), then the scheduler's tail
        with no guidance of its own. The momentum plane is allocated zeroed here and lives for the call.

        ``edit_embeds``: [n, T, D], one embedding per concept used for every sample, or [n, B, T, D]. The batch is always
        CONCEPT-MAJOR, the order the reference's string path builds (:426). Its ``editing_prompt_embeddings.tile([batch, 1, 1])``
        (:445) interleaves the concepts for B > 1 and then chunks them as if concept-major; that is not reproduced. The reference's
        per-step CPU copies (``uncond_estimates``, ``text_estimates``, ``edit_estimates``, ``sem_guidance[i]``) are not kept."""
        from .export import ExportedProgram
        if isinstance(self.unet, ExportedProgram):
            raise NotImplementedError("an exported program as `unet` together with editing prompts (semantic guidance) is not "
                                      "implemented: the exporter does not plan `mi355x_sd_sega_guidance`")
        if guidance_scale <= 1.0:
            raise NotImplementedError("editing prompts (semantic guidance) need `guidance_scale` > 1: without classifier-free "
                                      "guidance the reference silently ignores them")
        cfg, sch = self.unet.config, self.scheduler
        if getattr(cfg, "time_cond_proj_dim", None) is not None:
            raise NotImplementedError("a guidance-distilled U-Net (`time_cond_proj_dim`) together with editing prompts (semantic "
                                      "guidance) is not implemented")
        if getattr(cfg, "addition_embed_type", None) is not None or self.text_encoder_2 is not None:
            raise NotImplementedError("a U-Net with added conditioning (`addition_embed_type`: SDXL) together with editing prompts "
                                      "(semantic guidance) is not implemented: the reference has no such pipeline")
        lib, emulated = getattr(self.unet, "_lib", None), getattr(self.unet, "_emulated", False)
        if lib is None:
            raise _lib.MI355XError("semantic guidance runs its kernel through the U-Net's library: the `unet` has none")
        if not hasattr(lib, "mi355x_sd_sega_guidance"):
            raise _lib.MI355XError("the U-Net's library has no `mi355x_sd_sega_guidance` (ABI 25)")
        prompt_ids, negative_prompt_ids, edit_ids = ids
        if prompt_embeds is None:
            if prompt_ids is None:
                raise ValueError("Provide either `prompt_embeds` or `prompt_ids`")
            prompt_embeds = self.encode_prompt(prompt_ids)[0]
        if negative_prompt_embeds is None:
            if negative_prompt_ids is None:
                raise ValueError("classifier-free guidance needs `negative_prompt_embeds` (or `negative_prompt_ids`)")
            negative_prompt_embeds = self.encode_prompt(negative_prompt_ids)[0]
        if edit_embeds is None:
            edit_embeds = self.encode_prompt(edit_ids)[0]
        B = prompt_embeds.shape[0]
        if edit_embeds.dim() == 3:
            edit_embeds = edit_embeds[:, None].expand(-1, B, -1, -1)
        if edit_embeds.dim() != 4 or edit_embeds.shape[1] != B or edit_embeds.shape[2:] != prompt_embeds.shape[1:]:
            raise ValueError(f"`editing_prompt_embeds`: expected [n, T, D] or [n, {B}, T, D] with the prompt's T and D, got "
                             f"{tuple(edit_embeds.shape)}")
        n = edit_embeds.shape[0]
        embeds = torch.cat([negative_prompt_embeds, prompt_embeds, edit_embeds.reshape((n * B,) + tuple(prompt_embeds.shape[1:]))])
        h = (height // vae_scale_factor) if height else cfg.sample_size
        w = (width // vae_scale_factor) if width else cfg.sample_size
        if latents is not None and height is None and width is None:
            h, w = latents.shape[-2:]
        sch.set_timesteps(num_inference_steps)
        timesteps = sch.timesteps
        latents = self.prepare_latents(B, cfg.in_channels, h, w, torch.float32, generator, latents, prompt_embeds.device)
        dev, C = latents.device, latents.shape[1]
        table = sega_forms.rows(len(timesteps), n, h * w, guidance_scale, edit_momentum_scale, edit_mom_beta, **per_concept)
        extras = None
        if sem_guidance is not None:
            extras = (sem_guidance if torch.is_tensor(sem_guidance) else torch.stack(list(sem_guidance))).to(dev, torch.float32).contiguous()
            if extras.shape[0] < len(timesteps) or tuple(extras.shape[1:]) != tuple(latents.shape):
                raise ValueError(f"`sem_guidance`: expected at least {len(timesteps)} planes of shape {tuple(latents.shape)}, got "
                                 f"{tuple(extras.shape)}")
        step_params = inspect.signature(sch.step).parameters
        extra = {}
        if "eta" in step_params:
            extra["eta"] = eta
        if "generator" in step_params:
            extra["generator"] = generator
        tail = (self._fused_plan(False, dev, timesteps, generator) if fused_update and not eta else None) or _GenericTail(sch, extra)
        momentum = torch.zeros_like(latents)
        rows = torch.from_numpy(table.view(np.int32)).to(dev) if fused_guidance else None
        stride = 4 * sega_forms.row_words(n)
        for i, t in enumerate(timesteps):
            lat = latents.contiguous()
            model_input = tail.scale(torch.cat([lat] * (2 + n)), i, t)
            raw = self.unet(model_input, t, encoder_hidden_states=embeds, return_dict=False)[0].contiguous()
            ex = None if extras is None else extras[i]
            if fused_guidance:
                e = torch.empty_like(lat)
                _lib.check(lib.mi355x_sd_sega_guidance(raw.data_ptr(), momentum.data_ptr(), None if ex is None else ex.data_ptr(),
                                                       rows.data_ptr() + stride * i, e.data_ptr(), None, n, B, C, h * w,
                                                       program.caller_stream(dev, emulated)))
            else:
                e, momentum = self.semantic_guidance_torch(i, raw, n, momentum, ex, guidance_scale, edit_momentum_scale, edit_mom_beta,
                                                           per_concept)
            latents = tail.update(lat, e.contiguous(), i, t, False, 1.0, 0.0)
            if callback_on_step_end is not None:
                out = callback_on_step_end(self, i, t, {"latents": latents})
                latents = out.pop("latents", latents)
        if output_type == "latent":
            return latents
        return self.decode_latents(latents, output_type)

    @staticmethod
    def view_input_torch(x, views, circular):
        """The latents of `views` (rows of panorama_forms.views) stacked view-major, in the reference's expressions
        (pipeline_stable_diffusion_panorama.py:675-698): what ``mi355x_sd_view_input`` replaces at scale 1 and one group"""
        W, out = x.shape[3], []
        for h0, h1, w0, w1 in views:
            if circular and w1 > W:
                out.append(torch.cat((x[:, :, h0:h1, w0:], x[:, :, h0:h1, :w1 - W]), dim=-1))
            else:
                out.append(x[:, :, h0:h1, w0:w1])
        return torch.cat(out)

    @staticmethod
    def view_merge_torch(denoised, views, shape, circular):
        """``value`` / ``count`` / ``where`` of the reference (:736-754) on the device of `denoised` [len(views) * B, C, win_h, win_w]:
        what ``mi355x_sd_view_merge`` replaces"""
        value = torch.zeros(shape, dtype=denoised.dtype, device=denoised.device)
        count = torch.zeros_like(value)
        W = shape[3]
        for d, (h0, h1, w0, w1) in zip(denoised.chunk(len(views)), views):
            if circular and w1 > W:
                value[:, :, h0:h1, w0:] += d[:, :, :, :W - w0]
                value[:, :, h0:h1, :w1 - W] += d[:, :, :, W - w0:]
                count[:, :, h0:h1, w0:] += 1
                count[:, :, h0:h1, :w1 - W] += 1
            else:
                value[:, :, h0:h1, w0:w1] += d
                count[:, :, h0:h1, w0:w1] += 1
        return torch.where(count > 0, value / count, value)

    def _panorama(self, prompt_embeds, negative_prompt_embeds, num_inference_steps, guidance_scale, latents, generator,
                  callback_on_step_end, vae_scale_factor, output_type, ids, height, width, fused_update, eta, view_batch_size,
                  circular_padding, fused_views):
        """The loop of StableDiffusionPanoramaPipeline.__call__ (pipeline_stable_diffusion_panorama.py:589-783; MultiDiffusion). Every
        step cuts the latents into overlapping windows of panorama_forms.WINDOW at panorama_forms.STRIDE (``get_views``, :473-491),
        denoises every view with scheduler state of its own and averages the results per element. Per step and chunk of
        ``view_batch_size`` views (default: all of them): ONE ``mi355x_sd_view_input`` (a second one, unscaled, for the tail's sample
        where the scheduler scales its model input), ONE U-Net call on ``[negative x views | text x views]``, the scheduler's fused
        tail over the chunk's stacked views -- every tail is elementwise with its history in planes it owns, one tail object per
        chunk, so that is the reference's per-view-batch ``views_scheduler_status`` with no copy of any scheduler -- then ONE
        ``mi355x_sd_view_merge`` for the step. ``fused_update=False`` keeps ``scheduler.step`` with one copied scheduler state per
        chunk, as the reference does; ``fused_views=False`` takes the same step with the reference's torch expressions for the two
        passes. A latent smaller than the window on an axis clips the window to it.

        Departures from the reference. (1) Above batch 1 it interleaves the latents (``repeat_interleave(2)``) but tiles the
        embeddings ``[neg_0 .. neg_B-1, text_0 .. text_B-1]``: image 0 meets a negative prompt in both guidance halves, image 1 a
        text prompt in both, which is no guidance at all, even for one prompt repeated over the batch. Here every image goes with
        its own two prompts, in this library's group-major ``[uncond | text]`` order. The two agree at batch 1 and, at any batch,
        without guidance. (2) ``view_batch_size`` only chunks the U-Net calls: for the schedulers accepted here the
        reference's result does not depend on it either. Schedulers that draw noise are refused: the reference draws one tensor per
        view batch, so its result depends on ``view_batch_size`` and nothing pins a stacked draw."""
        import copy
        from .export import ExportedProgram
        if isinstance(self.unet, ExportedProgram):
            raise NotImplementedError("an exported program as `unet` together with `panorama` is not implemented: the exporter does "
                                      "not plan `mi355x_sd_view_input` / `mi355x_sd_view_merge`")
        cfg, sch = self.unet.config, self.scheduler
        if getattr(cfg, "time_cond_proj_dim", None) is not None:
            raise NotImplementedError("a guidance-distilled U-Net (`time_cond_proj_dim`) together with `panorama` is not implemented")
        if getattr(cfg, "addition_embed_type", None) is not None or self.text_encoder_2 is not None:
            raise NotImplementedError("a U-Net with added conditioning (`addition_embed_type`: SDXL) together with `panorama` is not "
                                      "implemented: the reference has no such pipeline")
        step_params = inspect.signature(sch.step).parameters
        if hasattr(sch, "ancestral_coefficients") or (hasattr(sch, "dpm2_coefficients") and "generator" in step_params) or \
                str(getattr(sch.config, "algorithm_type", "")).startswith("sde") or type(sch).__name__ == "LCMScheduler" or \
                (eta and "eta" in step_params):
            raise NotImplementedError(f"a scheduler that draws noise in its step ({type(sch).__name__}"
                                      f"{', eta > 0' if eta and 'eta' in step_params else ''}) together with `panorama` is not "
                                      "implemented: the reference draws one noise tensor per view batch, so its result depends on "
                                      "`view_batch_size`")
        lib, emulated = getattr(self.unet, "_lib", None), getattr(self.unet, "_emulated", False)
        if lib is None:
            raise _lib.MI355XError("`panorama` runs its view kernels through the U-Net's library: the `unet` has none")
        if fused_views and not (hasattr(lib, "mi355x_sd_view_input") and hasattr(lib, "mi355x_sd_view_merge")):
            raise _lib.MI355XError("the U-Net's library has no `mi355x_sd_view_input` / `mi355x_sd_view_merge` (ABI 26)")
        do_cfg = guidance_scale > 1.0
        prompt_ids, negative_prompt_ids = ids
        if prompt_embeds is None:
            if prompt_ids is None:
                raise ValueError("Provide either `prompt_embeds` or `prompt_ids`")
            prompt_embeds = self.encode_prompt(prompt_ids)[0]
        if do_cfg and negative_prompt_embeds is None:
            if negative_prompt_ids is None:
                raise ValueError("classifier-free guidance needs `negative_prompt_embeds` (or `negative_prompt_ids`)")
            negative_prompt_embeds = self.encode_prompt(negative_prompt_ids)[0]
        B = prompt_embeds.shape[0]
        h = (height // vae_scale_factor) if height else cfg.sample_size
        w = (width // vae_scale_factor) if width else cfg.sample_size
        if latents is not None and height is None and width is None:
            h, w = latents.shape[-2:]
        window, stride = panorama_forms.WINDOW, panorama_forms.STRIDE
        ny, nx, wh, ww = panorama_forms.grid(h, w, window, stride, circular_padding)
        if circular_padding and ny > 1:
            raise NotImplementedError("`circular_padding` with more than one row of views is not implemented: the reference itself "
                                      "fails there (it slices the view's own rows by the view's place in the panorama)")
        if circular_padding and w < window:
            raise NotImplementedError("`circular_padding` with latents narrower than the window is not implemented")
        views = panorama_forms.views(h, w, window, stride, circular_padding)
        total = len(views)
        per = total if view_batch_size is None else int(view_batch_size)
        if per < 1:
            raise ValueError(f"`view_batch_size` has to be a positive integer or None (all views), got {view_batch_size}")
        chunks = [(f, min(per, total - f)) for f in range(0, total, per)]
        sch.set_timesteps(num_inference_steps)
        timesteps = sch.timesteps
        latents = self.prepare_latents(B, cfg.in_channels, h, w, torch.float32, generator, latents, prompt_embeds.device)
        dev, C = latents.device, latents.shape[1]
        groups = 2 if do_cfg else 1
        embeds = {}
        for c in {c for _, c in chunks}:   # sample (v - first) * B + b of a group goes with prompt b
            text = prompt_embeds.repeat(c, 1, 1)
            embeds[c] = torch.cat([negative_prompt_embeds.repeat(c, 1, 1), text]) if do_cfg else text
        extra = {}
        if "eta" in step_params:
            extra["eta"] = eta
        if "generator" in step_params:
            extra["generator"] = generator
        tail = (self._fused_plan(False, dev, timesteps, generator) if fused_update and not eta else None) or _GenericTail(sch, extra)
        fused = isinstance(tail, _FusedTail)
        tails = [copy.copy(tail) for _ in chunks]                   # (a fused tail builds the state it owns on its first launch)
        status = None if fused else [copy.deepcopy(sch.__dict__) for _ in chunks]   # (:651)
        geo = (B, C, h, w, wh, ww, stride, ny, nx, int(bool(circular_padding)))
        stack = torch.empty((total * B, C, wh, ww), dtype=torch.float32, device=dev)      # the views of the latents, unscaled
        denoised = torch.empty_like(stack)
        model_in = {c: torch.empty((groups * c * B, C, wh, ww), dtype=torch.float32, device=dev) for c in embeds} if fused_views else None
        gs = float(guidance_scale)
        for i, t in enumerate(timesteps):
            stream = program.caller_stream(dev, emulated)
            lat = latents.contiguous()
            for j, (f, c) in enumerate(chunks):
                tl, n = tails[j], c * B
                if fused:
                    src, scale = lat, (1.0 if tl.scales is None else float(tl.scales[i]))
                else:   # the scheduler's own ``scale_model_input`` on the whole latents (elementwise: the windows' bits), in this chunk's state
                    sch.__dict__.update(status[j])
                    src, scale = tl.scale(lat, i, t).contiguous(), 1.0
                xs = stack[f * B:f * B + n]
                if fused_views:
                    x_in = model_in[c]
                    _lib.check(lib.mi355x_sd_view_input(src.data_ptr(), x_in.data_ptr(), scale, groups, *geo, f, c, stream))
                    if src is lat and scale == 1.0:
                        xs = x_in[:n]                               # (x * 1.0f is x: the first group is the tail's sample)
                    else:
                        _lib.check(lib.mi355x_sd_view_input(lat.data_ptr(), xs.data_ptr(), 1.0, 1, *geo, f, c, stream))
                else:
                    xs = self.view_input_torch(lat, views[f:f + c], circular_padding)
                    scaled = xs * scale if src is lat else self.view_input_torch(src, views[f:f + c], circular_padding)
                    x_in = torch.cat([scaled] * groups)
                e = self.unet(x_in, t, encoder_hidden_states=embeds[c], return_dict=False)[0].contiguous()
                if fused:
                    _lib.check(tl.launch(xs, e.data_ptr(), e.data_ptr() + 4 * xs.numel() if do_cfg else None, denoised[f * B:f * B + n],
                                         i, gs, 0.0, stream))
                else:
                    denoised[f * B:f * B + n] = tl.update(xs, e, i, t, do_cfg, guidance_scale, 0.0)
                    status[j] = copy.deepcopy(sch.__dict__)         # (:733)
            if fused_views:
                latents = torch.empty_like(lat)
                _lib.check(lib.mi355x_sd_view_merge(denoised.data_ptr(), latents.data_ptr(), *geo, stream))
            else:
                latents = self.view_merge_torch(denoised, views, lat.shape, circular_padding)
            if callback_on_step_end is not None:
                out = callback_on_step_end(self, i, t, {"latents": latents})
                latents = out.pop("latents", latents)
        if output_type == "latent":
            return latents
        return self.decode_latents(latents, output_type, circular_padding=bool(circular_padding))

    @torch.no_grad()
    def __call__(self, prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                 height: Optional[int] = None, width: Optional[int] = None, num_inference_steps: int = 50,
                 guidance_scale: float = 7.5, guidance_rescale: float = 0.0, latents: Optional[torch.Tensor] = None,
                 generator=None, added_cond_kwargs: Optional[Dict[str, torch.Tensor]] = None,
                 negative_added_cond_kwargs: Optional[Dict[str, torch.Tensor]] = None,
                 callback_on_step_end: Optional[Callable] = None, vae_scale_factor: int = 8,
                 output_type: str = "latent", prompt_ids: Optional[torch.Tensor] = None,
                 negative_prompt_ids: Optional[torch.Tensor] = None, prompt_ids_2: Optional[torch.Tensor] = None,
                 negative_prompt_ids_2: Optional[torch.Tensor] = None, original_size=None,
                 crops_coords_top_left=(0, 0), target_size=None, fused_update: bool = True,
                 image: Optional[torch.Tensor] = None, strength: Optional[float] = None, eta: float = 0.0,
                 mask_image: Optional[torch.Tensor] = None, masked_image_latents: Optional[torch.Tensor] = None,
                 control_image: Optional[torch.Tensor] = None, controlnet_conditioning_scale: float = 1.0,
                 guess_mode: bool = False, adapter_image=None, adapter_conditioning_scale=1.0,
                 adapter_conditioning_factor: float = 1.0, image_guidance_scale: Optional[float] = None,
                 editing_prompt_embeds: Optional[torch.Tensor] = None, editing_prompt_ids: Optional[torch.Tensor] = None,
                 reverse_editing_direction=False, edit_guidance_scale=5, edit_warmup_steps=10, edit_cooldown_steps=None,
                 edit_threshold=0.9, edit_momentum_scale: float = 0.1, edit_mom_beta: float = 0.4, edit_weights=None,
                 sem_guidance=None, fused_guidance: bool = True, panorama: bool = False, view_batch_size: Optional[int] = None,
                 circular_padding: bool = False, fused_views: bool = True):
        """``image`` (extension of the text2img call = StableDiffusionImg2ImgPipeline.__call__,
        pipeline_stable_diffusion_img2img.py:735-1010): start from the encoded, re-noised image and run the last
        ``int(num_inference_steps * strength)`` steps (strength defaults to 0.8).

        ``image`` + ``mask_image`` [B|1, 1, H, W] in [0, 1], 1 = repaint (= StableDiffusionInpaintPipeline.__call__,
        pipeline_stable_diffusion_inpaint.py:1094-1236; strength defaults to 1.0): a 9-channel UNet gets
        ``[latents | mask | masked-image latents]`` every step, a 4-channel UNet has the kept region re-imposed after every
        step from the re-noised image latents.

        ``adapter_image`` (= StableDiffusionAdapterPipeline / StableDiffusionXLAdapterPipeline.__call__,
        pipelines/t2i_adapter/pipeline_stable_diffusion_adapter.py:748-854, pipeline_stable_diffusion_xl_adapter.py:958-1032): fp32 NCHW
        in [0, 1], or a list of such images for a MultiAdapter. The adapter runs once before the loop; its features, times
        ``adapter_conditioning_scale`` (a list for a MultiAdapter: its ``adapter_weights``), repeated to the prompt batch and doubled
        under classifier-free guidance, go to the U-Net as ``down_intrablock_additional_residuals`` on the steps
        ``i < int(num_inference_steps * adapter_conditioning_factor)``; the other steps run the plain plan. Height and width default
        to the image's, floored to a multiple of ``adapter.downscale_factor``.

        ``image`` + ``image_guidance_scale`` (= StableDiffusionInstructPix2PixPipeline / StableDiffusionXLInstructPix2PixPipeline
        .__call__): instruction-based editing on an 8-channel U-Net, see ``_instruct_pix2pix``. ``strength`` is not used.

        ``editing_prompt_embeds`` / ``editing_prompt_ids`` (= SemanticStableDiffusionPipeline.__call__,
        pipelines/semantic_stable_diffusion/pipeline_semantic_stable_diffusion.py:225-727): semantic guidance, see
        ``_semantic_guidance``; the ``edit_*`` arguments and ``sem_guidance`` are the reference's, with its defaults and its
        scalar-or-list rules. ``fused_guidance=False`` takes the same step with torch ops.

        ``panorama=True`` (= StableDiffusionPanoramaPipeline.__call__, pipeline_stable_diffusion_panorama.py:495-783): MultiDiffusion
        over overlapping 64 x 64 latent windows at stride 8, see ``_panorama``. ``view_batch_size``: the views per U-Net call (None:
        all of them; the reference's default is 1); ``circular_padding``: the windows wrap around the right edge, and a non-latent
        output is decoded with wrapped padding; ``fused_views=False`` takes the same step with torch ops for the two view passes."""
        if panorama:
            for name, v in (("guidance_rescale", guidance_rescale or None), ("image_guidance_scale", image_guidance_scale),
                            ("image", image), ("mask_image", mask_image), ("control_image", control_image),
                            ("adapter_image", adapter_image), ("added_cond_kwargs", added_cond_kwargs),
                            ("editing_prompt_embeds", editing_prompt_embeds), ("editing_prompt_ids", editing_prompt_ids)):
                if v is not None:
                    raise NotImplementedError(f"`{name}` together with `panorama` is not implemented")
            return self._panorama(prompt_embeds, negative_prompt_embeds, num_inference_steps, guidance_scale, latents, generator,
                                  callback_on_step_end, vae_scale_factor, output_type, (prompt_ids, negative_prompt_ids), height, width,
                                  fused_update, eta, view_batch_size, circular_padding, fused_views)
        if editing_prompt_embeds is not None or editing_prompt_ids is not None:
            for name, v in (("guidance_rescale", guidance_rescale or None), ("image_guidance_scale", image_guidance_scale),
                            ("image", image), ("mask_image", mask_image), ("control_image", control_image),
                            ("adapter_image", adapter_image), ("added_cond_kwargs", added_cond_kwargs)):
                if v is not None:
                    raise NotImplementedError(f"`{name}` together with editing prompts (semantic guidance) is not implemented")
            return self._semantic_guidance(
                prompt_embeds, negative_prompt_embeds, editing_prompt_embeds, num_inference_steps, guidance_scale, latents, generator,
                callback_on_step_end, vae_scale_factor, output_type, (prompt_ids, negative_prompt_ids, editing_prompt_ids), height,
                width, fused_update, eta, fused_guidance, sem_guidance,
                dict(reverse_editing_direction=reverse_editing_direction, edit_guidance_scale=edit_guidance_scale,
                     edit_warmup_steps=edit_warmup_steps, edit_cooldown_steps=edit_cooldown_steps, edit_threshold=edit_threshold,
                     edit_weights=edit_weights), edit_momentum_scale, edit_mom_beta)
        if image_guidance_scale is not None:
            for name, v in (("mask_image", mask_image), ("control_image", control_image), ("adapter_image", adapter_image)):
                if v is not None:
                    raise NotImplementedError(f"`{name}` together with `image_guidance_scale` (InstructPix2Pix) is not implemented")
            return self._instruct_pix2pix(
                prompt_embeds, negative_prompt_embeds, image, num_inference_steps, guidance_scale, image_guidance_scale,
                guidance_rescale, latents, generator, added_cond_kwargs, negative_added_cond_kwargs, callback_on_step_end,
                vae_scale_factor, output_type, (prompt_ids, negative_prompt_ids, prompt_ids_2, negative_prompt_ids_2), original_size,
                crops_coords_top_left, target_size, fused_update, eta)
        inpaint = mask_image is not None
        adapter_hw = None
        if adapter_image is not None:
            if self.adapter is None:
                raise ValueError("`adapter_image` needs an `adapter`")
            if control_image is not None:
                raise NotImplementedError("a T2I-Adapter and a ControlNet in one call are not implemented")
            first = adapter_image if torch.is_tensor(adapter_image) else adapter_image[0]
            f = self.adapter.downscale_factor   # _default_height_width (pipeline_stable_diffusion_adapter.py:572-597)
            adapter_hw = ((height or first.shape[-2]) // f * f, (width or first.shape[-1]) // f * f)
            if latents is None or height is not None or width is not None:
                height, width = adapter_hw
        if inpaint and image is None:
            raise ValueError("`mask_image` needs `image`")
        if strength is None:
            strength = 1.0 if inpaint else 0.8
        # guidance-distilled UNets (LCM) take the scale as an embedding instead of a doubled batch (:634-635, :846-852)
        tc_dim = getattr(self.unet.config, "time_cond_proj_dim", None)
        do_cfg = guidance_scale > 1.0 and tc_dim is None
        if image is not None and (strength < 0 or strength > 1):
            raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
        if prompt_embeds is None:
            if prompt_ids is None:
                raise ValueError("Provide either `prompt_embeds` or `prompt_ids`")
            prompt_embeds, pooled = self.encode_prompt(prompt_ids, prompt_ids_2)
            neg_pooled = None
            if do_cfg and negative_prompt_embeds is None:
                if negative_prompt_ids is None:
                    # SDXL only: force_zeros_for_empty_prompt (pipeline_stable_diffusion_xl.py:378-381). The single-encoder
                    # pipelines encode the empty prompt "" through the text encoder instead (pipeline_stable_diffusion.py:409-441),
                    # and the tokenizer is not part of this path -> the caller must pass its token ids.
                    if self.text_encoder_2 is None:
                        raise ValueError("classifier-free guidance on a single-encoder pipeline needs `negative_prompt_ids` "
                                         "(the tokenised \"\" of the reference) or `negative_prompt_embeds`")
                    negative_prompt_embeds = torch.zeros_like(prompt_embeds)
                    neg_pooled = None if pooled is None else torch.zeros_like(pooled)
                else:
                    negative_prompt_embeds, neg_pooled = self.encode_prompt(negative_prompt_ids, negative_prompt_ids_2)
            if pooled is not None and added_cond_kwargs is None:   # SDXL micro-conditioning (:1007-1036)
                hw = (height or self.unet.config.sample_size * vae_scale_factor,
                      width or self.unet.config.sample_size * vae_scale_factor)
                tids = self.get_add_time_ids(tuple(original_size or hw), tuple(crops_coords_top_left),
                                             tuple(target_size or hw), pooled.shape[-1], pooled.device)
                tids = tids.repeat(pooled.shape[0], 1)
                added_cond_kwargs = {"text_embeds": pooled, "time_ids": tids}
                if do_cfg:
                    negative_added_cond_kwargs = {"text_embeds": neg_pooled, "time_ids": tids}
        if do_cfg and negative_prompt_embeds is None:
            raise ValueError("classifier-free guidance needs `negative_prompt_embeds`")
        B = prompt_embeds.shape[0]
        cfg = self.unet.config
        h = (height // vae_scale_factor) if height else cfg.sample_size
        w = (width // vae_scale_factor) if width else cfg.sample_size
        if latents is not None and height is None and width is None:
            h, w = latents.shape[-2:]
        if do_cfg:  # :813-814: [negative, positive]
            prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds])
            if added_cond_kwargs is not None:
                neg = negative_added_cond_kwargs or added_cond_kwargs
                added_cond_kwargs = {k: torch.cat([neg[k], v]) for k, v in added_cond_kwargs.items()}
        import inspect
        # LatentConsistencyModelImg2ImgPipeline (pipeline_latent_consistency_img2img.py:760-764): a scheduler whose
        # set_timesteps takes `strength` (LCMScheduler) shortens its own distillation schedule and ALL num_inference_steps of it
        # run; every other scheduler keeps the SD img2img rule (the last int(steps * strength) entries, get_timesteps)
        lcm_strength = image is not None and "strength" in inspect.signature(self.scheduler.set_timesteps).parameters
        if lcm_strength:
            self.scheduler.set_timesteps(num_inference_steps, strength=strength)
        else:
            self.scheduler.set_timesteps(num_inference_steps)
        timesteps, first, inp = self.scheduler.timesteps, 0, None
        if image is not None:
            if not lcm_strength:
                timesteps, _, first = self.get_timesteps(num_inference_steps, strength)
            if len(timesteps) < 1:
                raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of "
                                 "pipeline steps is 0 which is < 1 and not appropriate for this pipeline.")
            if inpaint:
                latents, inp = self.prepare_inpaint(image, mask_image, masked_image_latents, timesteps, B, generator,
                                                    strength == 1.0, do_cfg)
            else:
                latents = self.prepare_image_latents(image, timesteps[:1], B, generator)
        else:
            latents = self.prepare_latents(B, cfg.in_channels, h, w, torch.float32, generator, latents, prompt_embeds.device)
        step_params = inspect.signature(self.scheduler.step).parameters   # prepare_extra_step_kwargs (:520-535)
        extra = {}
        if "eta" in step_params:
            extra["eta"] = eta
        if "generator" in step_params:
            extra["generator"] = generator
        unet_kw = {}
        if tc_dim is not None:
            w = torch.full((B,), float(guidance_scale) - 1.0, device=latents.device)
            unet_kw["timestep_cond"] = self.get_guidance_scale_embedding(w, embedding_dim=tc_dim)
        rescale = do_cfg and guidance_rescale > 0.0   # without CFG the reference applies no rescale (:886-888)
        tail = (self._fused_plan(rescale, latents.device, timesteps, generator) if fused_update and not eta else None) \
            or _GenericTail(self.scheduler, extra)
        guidance = (do_cfg, guidance_scale, guidance_rescale if rescale else 0.0)
        nine = inp is not None and cfg.in_channels != latents.shape[1]
        adapter_state = None
        if adapter_image is not None:
            adapter_state = self._adapter_state(adapter_image, adapter_hw, adapter_conditioning_scale, B, do_cfg)
        adapter_steps = int(num_inference_steps * adapter_conditioning_factor)

        def adapt(i):
            """this step's T2I-Adapter residuals: a fresh list every step, withheld from step int(n * factor) on"""
            if adapter_state is None or i >= adapter_steps:
                return {}
            return dict(down_intrablock_additional_residuals=list(adapter_state))

        def control(x_in, t):
            """ControlNet residuals of this step (pipeline_controlnet.py:1148-1192): the ControlNet sees the UNet's input batch
            -- or, in guess mode under CFG, only the conditional half, the unconditional half getting zero residuals"""
            if control_image is None:
                return {}
            if self.controlnet is None:
                raise ValueError("`control_image` needs a `controlnet`")
            half = guess_mode and do_cfg
            pick = (lambda v: v.chunk(2)[1]) if half else (lambda v: v)
            img = control_image if (half or not do_cfg) else torch.cat([control_image] * 2)
            added = None if added_cond_kwargs is None else {k: pick(v) for k, v in added_cond_kwargs.items()}
            d, m = self.controlnet(pick(x_in)[:, :latents.shape[1]], t, encoder_hidden_states=pick(prompt_embeds),
                                   controlnet_cond=img, conditioning_scale=controlnet_conditioning_scale,
                                   guess_mode=guess_mode, added_cond_kwargs=added, return_dict=False)
            if half:
                d, m = tuple(torch.cat([torch.zeros_like(x), x]) for x in d), torch.cat([torch.zeros_like(m), m])
            return dict(down_block_additional_residuals=d, mid_block_additional_residual=m)

        def extend(x):   # 9-channel inpainting UNet: [scaled latents | mask | masked-image latents] (:1194-1198)
            return torch.cat([x, inp["mask_in"], inp["masked_in"]], dim=1) if nine else x

        def reimpose(lat, step_no):   # 4-channel UNet: keep the unmasked region on the re-noised image latents (:1218-1231)
            if inp is None or nine:
                return lat
            proper = inp["image_latents"]
            if step_no < len(timesteps) - 1:
                nt = torch.as_tensor(np.asarray(timesteps[step_no + 1]).reshape(1)).repeat(proper.shape[0])
                proper = self.scheduler.add_noise(proper, inp["noise"], nt)
            return (1 - inp["mask"]) * proper + inp["mask"] * lat

        for i, t in enumerate(timesteps, start=first):
            model_input = tail.scale(torch.cat([latents] * 2) if do_cfg else latents, i, t)
            noise_pred = self.unet(extend(model_input), t, encoder_hidden_states=prompt_embeds, added_cond_kwargs=added_cond_kwargs,
                                   return_dict=False, **unet_kw, **control(model_input, t), **adapt(i))[0]
            latents = reimpose(tail.update(latents, noise_pred, i, t, *guidance), i - first)
            if callback_on_step_end is not None:
                out = callback_on_step_end(self, i, t, {"latents": latents})
                latents = out.pop("latents", latents)
        if output_type == "latent":
            return latents
        return self.decode_latents(latents, output_type)


class StableDiffusion3Denoiser(_VaeSwitches):
    """The denoising loop of ``StableDiffusion3Pipeline.__call__`` (pipelines/stable_diffusion_3/
    pipeline_stable_diffusion_3.py:772-870) with the MI355X MMDiT in the ``transformer`` slot: CFG batch doubling
    ([negative, positive]), the transformer call, the guidance combine, ``FlowMatchEulerDiscreteScheduler.step`` and
    ``callback_on_step_end``; then (:880-886) ``vae.decode(latents / scaling_factor + shift_factor)``.
    Prompt encoding (2 x CLIP + T5) stays outside: the loop takes ``prompt_embeds`` [B, L, joint_attention_dim] and
    ``pooled_prompt_embeds`` [B, pooled_projection_dim]."""

    def __init__(self, transformer, scheduler, vae=None, text_encoder=None, text_encoder_2=None, text_encoder_3=None):
        self.transformer, self.scheduler, self.vae = transformer, scheduler, vae
        self.text_encoder, self.text_encoder_2, self.text_encoder_3 = text_encoder, text_encoder_2, text_encoder_3

    def encode_prompt(self, input_ids: torch.Tensor, input_ids_2: torch.Tensor, input_ids_3: torch.Tensor,
                      clip_skip: Optional[int] = None):
        """Token ids of the three tokenizers -> (prompt_embeds [B, S_clip + S_t5, joint_dim], pooled [B, P1 + P2]);
        pipeline_stable_diffusion_3.py:375-398: both CLIP encoders (with projection) contribute hidden_states[-2],
        concatenated on the channel axis and zero-padded to the T5 width, then the T5 sequence is appended on the token
        axis; pooled = the two projected EOS rows side by side."""
        if self.text_encoder is None or self.text_encoder_2 is None or self.text_encoder_3 is None:
            raise ValueError("encode_prompt needs `text_encoder`, `text_encoder_2` (CLIP with projection) and "
                             "`text_encoder_3` (T5)")
        embeds, pooled = [], []
        for enc, ids in ((self.text_encoder, input_ids), (self.text_encoder_2, input_ids_2)):
            out = enc(ids, output_hidden_states=True)
            pooled.append(out[0])
            embeds.append(out.hidden_states[-2 if clip_skip is None else -(clip_skip + 2)])
        clip = torch.cat(embeds, dim=-1)
        t5 = self.text_encoder_3(input_ids_3)[0]
        clip = torch.nn.functional.pad(clip, (0, t5.shape[-1] - clip.shape[-1]))
        return torch.cat([clip, t5], dim=-2), torch.cat(pooled, dim=-1)

    @torch.no_grad()
    def __call__(self, prompt_embeds: torch.Tensor, pooled_prompt_embeds: torch.Tensor,
                 negative_prompt_embeds: Optional[torch.Tensor] = None,
                 negative_pooled_prompt_embeds: Optional[torch.Tensor] = None, height: Optional[int] = None,
                 width: Optional[int] = None, num_inference_steps: int = 28, guidance_scale: float = 7.0,
                 latents: Optional[torch.Tensor] = None, generator=None, callback_on_step_end: Optional[Callable] = None,
                 vae_scale_factor: int = 8, output_type: str = "latent"):
        do_cfg = guidance_scale > 1.0
        if do_cfg and (negative_prompt_embeds is None or negative_pooled_prompt_embeds is None):
            raise ValueError("classifier-free guidance needs `negative_prompt_embeds` and `negative_pooled_prompt_embeds`")
        cfg = self.transformer.config
        B = prompt_embeds.shape[0]
        h = (height // vae_scale_factor) if height else cfg.sample_size
        w = (width // vae_scale_factor) if width else cfg.sample_size
        shape = (B, cfg.in_channels, h, w)
        if latents is None:
            latents = torch.randn(shape, generator=generator, dtype=torch.float32, device=prompt_embeds.device)
        elif height is None and width is None:
            shape = tuple(latents.shape)
        if tuple(latents.shape) != shape:
            raise ValueError(f"Unexpected latents shape, got {tuple(latents.shape)}, expected {shape}")
        if do_cfg:
            prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0)
            pooled_prompt_embeds = torch.cat([negative_pooled_prompt_embeds, pooled_prompt_embeds], dim=0)
        self.scheduler.set_timesteps(num_inference_steps)
        for i, t in enumerate(self.scheduler.timesteps):
            x = torch.cat([latents] * 2) if do_cfg else latents
            v = self.transformer(hidden_states=x, timestep=t, encoder_hidden_states=prompt_embeds,
                                 pooled_projections=pooled_prompt_embeds, return_dict=False)[0]
            if do_cfg:
                v_uncond, v_text = v.chunk(2)
                v = v_uncond + guidance_scale * (v_text - v_uncond)
            latents = self.scheduler.step(v, t, latents, return_dict=False)[0]
            if callback_on_step_end is not None:
                out = callback_on_step_end(self, i, t, {"latents": latents})
                latents = out.pop("latents", latents)
        if output_type == "latent":
            return latents
        return self._postprocess(output_type, lambda: self.vae.decode(
            latents / self.vae.config.scaling_factor + (getattr(self.vae.config, "shift_factor", None) or 0.0), return_dict=False)[0])


class DiTDenoiser(_VaeSwitches):
    """The loop of ``DiTPipeline.__call__`` (pipelines/dit/pipeline_dit.py:158-246) with the MI355X DiT in the ``transformer``
    slot: class-conditional classifier-free guidance with the null class (index ``num_embeds_ada_norm``) on the DUPLICATED
    latent half (:182-184), guidance applied to the epsilon channels only (:209-216), the learned-sigma channels dropped
    before ``scheduler.step`` (:219-225), then ``vae.decode(latents / scaling_factor)`` and the denormalise (:235-246)."""

    def __init__(self, transformer, scheduler, vae=None):
        self.transformer, self.scheduler, self.vae = transformer, scheduler, vae

    @torch.no_grad()
    def __call__(self, class_labels, guidance_scale: float = 4.0, num_inference_steps: int = 50, generator=None,
                 latents: Optional[torch.Tensor] = None, output_type: str = "latent",
                 callback_on_step_end: Optional[Callable] = None, device=None):
        cfg = self.transformer.config
        labels = torch.as_tensor(class_labels).reshape(-1)
        device = device or (latents.device if latents is not None else labels.device)
        labels = labels.to(device)
        B, C, side = labels.numel(), cfg.in_channels, cfg.sample_size
        if latents is None:
            latents = torch.randn((B, C, side, side), generator=generator, dtype=torch.float32, device=device)
        elif tuple(latents.shape[:2]) != (B, C):
            raise ValueError(f"Unexpected latents shape, got {tuple(latents.shape)}, expected ({B}, {C}, h, w)")
        do_cfg = guidance_scale > 1
        x = torch.cat([latents] * 2) if do_cfg else latents
        null = torch.full((B,), cfg.num_embeds_ada_norm, dtype=labels.dtype, device=device)
        labels_in = torch.cat([labels, null]) if do_cfg else labels
        self.scheduler.set_timesteps(num_inference_steps)
        for i, t in enumerate(self.scheduler.timesteps):
            if do_cfg:
                half = x[: len(x) // 2]
                x = torch.cat([half, half], dim=0)
            x = self.scheduler.scale_model_input(x, t)
            ts = torch.as_tensor(t, device=device).reshape(-1).expand(x.shape[0])
            noise = self.transformer(x, timestep=ts, class_labels=labels_in, return_dict=False)[0]
            if do_cfg:
                eps, rest = noise[:, :C], noise[:, C:]
                cond, uncond = eps.chunk(2, dim=0)
                half_eps = uncond + guidance_scale * (cond - uncond)
                noise = torch.cat([torch.cat([half_eps, half_eps], dim=0), rest], dim=1)
            model_output = noise[:, :C] if cfg.out_channels // 2 == C else noise   # learned sigma is not used by the step
            x = self.scheduler.step(model_output, t, x, return_dict=False)[0]
            if callback_on_step_end is not None:
                x = callback_on_step_end(self, i, t, {"latents": x}).pop("latents", x)
        latents = x.chunk(2, dim=0)[0] if do_cfg else x
        if output_type == "latent":
            return latents
        return self._postprocess(output_type, lambda: self.vae.decode(
            latents, return_dict=False, in_scale=1.0 / self.vae.config.scaling_factor)[0])
