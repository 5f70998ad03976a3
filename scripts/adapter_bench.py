#!/usr/bin/env python
"""What the T2I-Adapter costs at the SDXL batch-8 geometry (bf16 elements unless MI355X_SD_DTYPE says otherwise):

  1. one adapter forward: full_adapter_xl with the reference's default channels on an 8 x 3 x 1024 x 1024 image -- graph replay, HIP
     events around one replay, median of REPS after WARM;
  2. the U-Net step (8 x 4 x 128 x 128 latents, 77 tokens) with the four intrablock adds against the same model's plain step:
     the two captured plans replayed in turn (A B A B ...), one pair of events per replay, median of REPS each, and the median of
     the per-pair differences; then the same through ``forward`` (which also stages the four fp32 residuals, 210 MB, every call).

Random weights (drawn on the device); times depend on shapes only.

    python scripts/adapter_bench.py > profiles/<name>.txt"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from paddlemix_amd import _lib   # noqa: E402
from paddlemix_amd.adapter import T2IAdapter, synth_adapter_params   # noqa: E402
from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params   # noqa: E402
from tests.configs import SDXL   # noqa: E402

B, H, W, L, WARM, REPS = 8, 128, 128, 77, 3, 15
ADAPTER = dict(in_channels=3, channels=(320, 640, 1280, 1280), num_res_blocks=2, downscale_factor=16, adapter_type="full_adapter_xl")


def event_ms(fn, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def med(v):
    return f"{statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f}, n = {len(v)})"


def main():
    dev = "cuda"
    print(f"# {_lib.ELEM_NAME} elements; B = {B}, latents {H} x {W}, {L} tokens; image {8 * H} x {8 * W}")
    adapter = T2IAdapter(ADAPTER, synth_adapter_params(ADAPTER, seed=21, device=dev))
    image = torch.rand(B, 3, 8 * H, 8 * W, device=dev)
    feats = adapter(image)
    plan = adapter._get_plan(B, 8 * H, 8 * W)
    print("adapter features: " + ", ".join("x".join(str(d) for d in f.shape) for f in feats) + f"; {len(plan.prog)} launches")
    with adapter.on_stream():
        for _ in range(WARM):
            adapter.run(plan)
        t = [event_ms(lambda: adapter.run(plan), adapter._stream) for _ in range(REPS)]
    print("adapter forward (graph replay, inputs staged): " + med(t))
    t = [event_ms(lambda: adapter(image), torch.cuda.current_stream()) for _ in range(REPS)]
    print("adapter forward (forward(): staging + replay + the clones of the four features): " + med(t))
    del adapter, plan
    torch.cuda.empty_cache()

    model = UNet2DConditionModel(SDXL, synth_unet_params(SDXL, seed=1234, device=dev))
    g = torch.Generator(device=dev).manual_seed(0)
    sample = torch.randn(B, 4, H, W, generator=g, device=dev)
    enc = torch.randn(B, L, SDXL["cross_attention_dim"], generator=g, device=dev)
    added = dict(text_embeds=torch.randn(B, 1280, generator=g, device=dev),
                 time_ids=torch.tensor([[1024., 1024., 0., 0., 1024., 1024.]], device=dev).repeat(B, 1))
    assert [tuple(f.shape) for f in feats] == model.intrablock_shapes(B, H, W)
    kw = dict(added_cond_kwargs=added)
    plain_out = model(sample, 501, enc, **kw).sample
    on_out = model(sample, 501, enc, down_intrablock_additional_residuals=feats, **kw).sample
    plans = list(model._plans.values())
    names = [[fn.__name__ for fn, *_ in p.prog] for p in plans]
    print(f"U-Net plans: plain {len(names[0])} launches, with the adapter {len(names[1])} launches "
          f"({sum(n.startswith('mi355x_sd_add_nchw') for n in names[1])} adds); the adds move the prediction by rel-L2 "
          f"{((on_out - plain_out).norm() / plain_out.norm()).item():.3f}")
    a, b, d = [], [], []
    with model.on_stream():
        for _ in range(WARM):
            model.run(plans[0]), model.run(plans[1])
        for _ in range(REPS):
            ta, tb = event_ms(lambda: model.run(plans[0]), model._stream), event_ms(lambda: model.run(plans[1]), model._stream)
            a.append(ta), b.append(tb), d.append(tb - ta)
    print("step, graph replay, plain:            " + med(a))
    print("step, graph replay, four adds:        " + med(b))
    print("  difference per interleaved pair:    " + med(d))
    a, b, d = [], [], []
    cur = torch.cuda.current_stream()
    for _ in range(REPS):
        ta = event_ms(lambda: model(sample, 501, enc, **kw), cur)
        tb = event_ms(lambda: model(sample, 501, enc, down_intrablock_additional_residuals=feats, **kw), cur)
        a.append(ta), b.append(tb), d.append(tb - ta)
    print("step, forward(), plain:               " + med(a))
    print("step, forward(), four residuals:      " + med(b))
    print("  difference per interleaved pair:    " + med(d))


if __name__ == "__main__":
    main()
