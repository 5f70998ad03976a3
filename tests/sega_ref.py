"""The reference's semantic-guidance loop restated line by line in torch, in the dtype of its inputs -- TEST INFRASTRUCTURE ONLY.

REF = ppdiffusers/ppdiffusers/pipelines/semantic_stable_diffusion/pipeline_semantic_stable_diffusion.py

It uses paddlemix_amd/schedulers.py's own classes for ``set_timesteps``, ``scale_model_input`` and ``step`` and takes the U-Net as a
callable, so it runs on the CPU against the emulated loop and the recorded loops (tests/golden/sega). ``torch.quantile`` stands where
the reference calls ``paddle.quantile`` (what oracle/paddle_shim.py maps it to). The per-step CPU copies the reference keeps
(``uncond_estimates`` ...) are not restated: nothing reads them. The edit embeddings are concept-major, [n * B, T, D]: what the
reference's string path builds (REF :426); its ``editing_prompt_embeddings.tile`` (REF :445) interleaves the concepts for B > 1 and
is not restated."""
import inspect

import torch


def guidance_step(i, noise_pred, n, guidance_scale, edit_momentum, reverse_editing_direction=False, edit_guidance_scale=5,
                  edit_warmup_steps=10, edit_cooldown_steps=None, edit_threshold=0.9, edit_momentum_scale=0.1, edit_mom_beta=0.4,
                  edit_weights=None, sem_guidance=None, seen=None):
    """REF :541-699 for one step: the U-Net output of (2 + n) * B samples -> (noise_pred, edit_momentum)"""
    noise_pred_out = noise_pred.chunk(2 + n)                                                          # :541
    noise_pred_uncond, noise_pred_text = noise_pred_out[0], noise_pred_out[1]
    noise_pred_edit_concepts = noise_pred_out[2:]
    noise_guidance = guidance_scale * (noise_pred_text - noise_pred_uncond)                           # :546
    if edit_momentum is None:
        edit_momentum = torch.zeros_like(noise_guidance)                                              # :566
    if n:
        concept_weights = torch.zeros((n, noise_guidance.shape[0]), dtype=noise_guidance.dtype)       # :569
        noise_guidance_edit = torch.zeros((n, *noise_guidance.shape), dtype=noise_guidance.dtype)     # :573
        warmup_inds = []
        for c, noise_pred_edit_concept in enumerate(noise_pred_edit_concepts):
            edit_guidance_scale_c = edit_guidance_scale[c] if isinstance(edit_guidance_scale, list) else edit_guidance_scale
            edit_threshold_c = edit_threshold[c] if isinstance(edit_threshold, list) else edit_threshold
            reverse_c = reverse_editing_direction[c] if isinstance(reverse_editing_direction, list) else reverse_editing_direction
            edit_weight_c = edit_weights[c] if edit_weights else 1.0
            edit_warmup_steps_c = edit_warmup_steps[c] if isinstance(edit_warmup_steps, list) else edit_warmup_steps
            if isinstance(edit_cooldown_steps, list):
                edit_cooldown_steps_c = edit_cooldown_steps[c]
            elif edit_cooldown_steps is None:
                edit_cooldown_steps_c = i + 1
            else:
                edit_cooldown_steps_c = edit_cooldown_steps
            if i >= edit_warmup_steps_c:
                warmup_inds.append(c)                                                                 # :609
            if i >= edit_cooldown_steps_c:
                noise_guidance_edit[c] = torch.zeros_like(noise_pred_edit_concept)                    # :611-613
                continue
            tmp = noise_pred_edit_concept - noise_pred_uncond                                         # :615
            if reverse_c:
                tmp = tmp * -1
            concept_weights[c, :] = edit_weight_c                                                     # :619-624
            tmp = tmp * edit_guidance_scale_c                                                         # :626
            thr = torch.quantile(torch.abs(tmp).flatten(2), edit_threshold_c, dim=2, keepdim=False)   # :630
            if seen is not None:
                seen.append((i, c, tmp.clone(), thr.clone()))
            tmp = torch.where(torch.abs(tmp) >= thr[:, :, None, None], tmp, torch.zeros_like(tmp))    # :644
            noise_guidance_edit[c] = tmp
        warm = torch.tensor(warmup_inds, dtype=torch.long)
        if n > warm.shape[0] > 0:                                                                     # :654
            cw = torch.index_select(concept_weights, 0, warm)
            cw = torch.where(cw < 0, torch.zeros_like(cw), cw)
            cw = cw / cw.sum(dim=0)
            tmp = torch.index_select(noise_guidance_edit, 0, warm)
            tmp = torch.einsum("cb,cbijk->bijk", cw, tmp)
            noise_guidance = noise_guidance + tmp                                                     # :670
        concept_weights = torch.where(concept_weights < 0, torch.zeros_like(concept_weights), concept_weights)
        concept_weights = torch.nan_to_num(concept_weights)                                           # :683
        noise_guidance_edit = torch.einsum("cb,cbijk->bijk", concept_weights, noise_guidance_edit)    # :685
        noise_guidance_edit = noise_guidance_edit + edit_momentum_scale * edit_momentum               # :687
        edit_momentum = edit_mom_beta * edit_momentum + (1 - edit_mom_beta) * noise_guidance_edit     # :689
        if warm.shape[0] == n:
            noise_guidance = noise_guidance + noise_guidance_edit                                     # :692
    if sem_guidance is not None:
        noise_guidance = noise_guidance + sem_guidance[i]                                             # :695-697
    return noise_pred_uncond + noise_guidance, edit_momentum                                          # :699


def loop(unet, scheduler, prompt_embeds, negative_prompt_embeds, edit_embeds, latents, num_inference_steps, guidance_scale,
         generator=None, on_step=None, seen=None, **edit):
    """-> the final latents. latents: the initial noise before init_noise_sigma; edit_embeds [n * B, T, D] concept-major, or None.
    on_step(i, t, latents_before, raw, noise_pred, edit_momentum) sees every step."""
    n = 0 if edit_embeds is None else edit_embeds.shape[0] // prompt_embeds.shape[0]
    assert guidance_scale > 1.0                                                                       # :455 (the product refuses the rest)
    text_embeddings = torch.cat([negative_prompt_embeds, prompt_embeds] + ([edit_embeds] if n else []))   # :497-499
    scheduler.set_timesteps(num_inference_steps)                                                      # :503
    latents = latents * scheduler.init_noise_sigma                                                    # :221
    extra = {"generator": generator} if "generator" in inspect.signature(scheduler.step).parameters else {}
    edit_momentum = None
    for i, t in enumerate(scheduler.timesteps):
        latent_model_input = torch.cat([latents] * (2 + n))                                           # :531
        latent_model_input = scheduler.scale_model_input(latent_model_input, t)                       # :534
        raw = unet(latent_model_input, t, encoder_hidden_states=text_embeddings, return_dict=False)[0]
        noise_pred, edit_momentum = guidance_step(i, raw, n, guidance_scale, edit_momentum, seen=seen, **edit)
        if on_step is not None:
            on_step(i, t, latents, raw, noise_pred, edit_momentum)
        latents = scheduler.step(noise_pred, t, latents, **extra, return_dict=False)[0]               # :702
    return latents
