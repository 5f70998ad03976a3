#!/usr/bin/env python
"""Headline benchmark: UNet denoising steps/sec, SD-XL base UNet, 1024x1024 (latents 8x4x128x128), bs=8 per GPU.

One "step" = scheduler.scale_model_input (folded into conv_in) + UNet2DConditionModel forward (hipGraph replay) +
Euler scheduler latent update, on synthetic inputs already resident in HBM; weights are random-init (no
checkpoints offline).  N>1: one process per GPU (torchrun), rank 0 generates the weights and RCCL-broadcasts them
over xGMI, every rank then denoises its own shard of 8 prompts with no per-step collective (weak scaling).

Prints ONE JSON line (see the field notes in DESIGN.md "Measurement").

A plain run sets up, warms up, times --steps steps, writes the last step's outputs when --dump-outputs DIR is given, and prints the
line. --full adds everything else the line can carry: the board clock / power sample (taken when --steps >= 20), the roofline
pass, the CPU baseline and the parity legs (the last three each switched off by its own --no-* option).
"""
import argparse
import contextlib
import json
import os
import socket
import sys
import time

# the host driver only supports dmabuf IPC: without this RCCL's peer buffers fail with hipIpcGetMemHandle "invalid argument"
# (read by the HSA runtime when the first HIP call initialises it, so it has to be in the environment before that)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SDXL = dict(block_out_channels=(320, 640, 1280), down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
            up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"),
            transformer_layers_per_block=(1, 2, 10), attention_head_dim=(5, 10, 20), cross_attention_dim=2048,
            use_linear_projection=True, addition_embed_type="text_time", addition_time_embed_dim=256,
            projection_class_embeddings_input_dim=2816, layers_per_block=2, sample_size=128)
SD15 = dict(block_out_channels=(320, 640, 1280, 1280), cross_attention_dim=768, attention_head_dim=8, layers_per_block=2,
            sample_size=64)
SD3_MEDIUM = dict(sample_size=128, patch_size=2, in_channels=16, num_layers=24, attention_head_dim=64,
                  num_attention_heads=24, caption_projection_dim=1536, joint_attention_dim=4096,
                  pooled_projection_dim=2048, out_channels=16, pos_embed_max_size=192)
CLIP_L = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
              max_position_embeddings=77, hidden_act="quick_gelu", projection_dim=768, eos_token_id=2)
CLIP_BIGG = dict(vocab_size=49408, hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=20,
                 max_position_embeddings=77, hidden_act="gelu", projection_dim=1280, eos_token_id=2, with_projection=True)
WORKLOADS = {
    "sdxl-1024-bs8": dict(cfg=SDXL, B=8, H=128, W=128, L=77, gflop_step=54089.8),
    "sd15-512-bs1": dict(cfg=SD15, B=1, H=64, W=64, L=77, gflop_step=803.3),
    # SD3-medium MMDiT, bf16 weights (fp8 weights: the -fp8w workload): FLOPs from the plan
    "sd3-1024-bs8": dict(cfg=SD3_MEDIUM, B=8, H=128, W=128, L=154, gflop_step=None, sd3=True),
    # BASELINE config 5: the same model with weight-only fp8 (e4m3 + per-channel scale) block matrices
    "sd3-1024-bs8-fp8w": dict(cfg=SD3_MEDIUM, B=8, H=128, W=128, L=154, gflop_step=None, sd3=True, fp8=True),
    # the same with fp8 activations into the block GEMMs: W8A8 on the fp8 matrix pipe (v_mfma_scale_f32_16x16x128_f8f6f4)
    "sd3-1024-bs8-w8a8": dict(cfg=SD3_MEDIUM, B=8, H=128, W=128, L=154, gflop_step=None, sd3=True, fp8=True, a8=True),
}
# tests/parity_cases.py: full SDXL parameter set, committed oracle trajectories -- 30 Euler steps at 1x4x32x32 and at 1x4x128x128 (one
# prompt of the headline geometry over the metric's whole schedule; its first ten steps are the 10-step fixture, not replayed here)
PARITY_CASES = ("sdxl_1x4x32x32_euler30", "sdxl_1x4x128x128_euler30")
PEAK_BF16_TFLOPS = 2500.0  # dense MFMA bf16 / fp16, MI355X_MICROARCH.md chip table
PEAK_FP8_TFLOPS = 5000.0   # dense MFMA fp8 (the W8A8 workload's block GEMMs)
DUMP_BYTES = 64 * 10**6     # --dump-outputs: at most this much in all


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)    # 3 warm-up + >= 30 timed steps (one Euler schedule)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="sdxl-1024-bs8", choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: board clock / power during the timed steps, "
                         "the roofline pass, the CPU baseline and the parity legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (latents after the scheduler update, the "
                         "model's noise prediction) as DIR/<name>.npy, float32; at most 64 MB in all (above that, a fixed seeded "
                         "sample of the batch rows)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--residual", default="16", choices=["16", "fp32"],
                    help="storage type of the residual stream (fp32: tighter parity, more HBM traffic; DESIGN.md section 4)")
    ap.add_argument("--text-encoders", action="store_true",
                    help="also build the two SDXL text encoders from broadcast weights and encode the prompts on every rank "
                         "(default for --gpus > 1: north_star's 'RCCL broadcast of text-encoder/UNet weights')")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"],
                    help="16-bit element type = which build of the library runs (bf16: BASELINE.json's configurations; "
                         "fp16: same MFMA rate, ~6x tighter parity)")
    ap.add_argument("--no-parity-mode", action="store_true",
                    help="skip the two parity legs: the live replay of the full-depth loops in the benchmarked mode, and the timed loop "
                         "+ replay in the cheapest mode that meets the 1e-3 latents bar (fp16 elements, 16-bit residual stream)")
    # test plumbing (tests/test_distributed.py): the launcher, the rendezvous, the barrier / max-over-ranks timing protocol and
    # the one-JSON-line contract on CPU ranks (gloo) with the C-ABI interpreter of tests/abi_emulator.py standing in for the
    # library on the tiny test UNet. The line it prints says "selftest": it is never a measurement.
    ap.add_argument("--selftest-cpu", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--force-dist", action="store_true",
                    help="run the multi-rank code path (RCCL process group, weight broadcast, text encoders from broadcast weights, "
                         "barriers, final all-gather) even with one rank: the N > 1 path on the one GPU a box has")
    # the child process of the parity legs (one element type per process; --dtype / --residual say which): the seeded weights of
    # tests/parity_cases.py, a timed loop at the headline geometry, then the full-depth replays against the committed oracle
    # trajectories (the checker: tests/ + tests/golden/, never part of a timed region)
    ap.add_argument("--parity-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--parity-cases", default=",".join(PARITY_CASES), help=argparse.SUPPRESS)
    return ap.parse_args()


def usable_cpus(cgroup_root: str = "/sys/fs/cgroup") -> int:
    """CPUs this process may actually use: its affinity mask, capped by the container's CPU quota (cgroup v2 `cpu.max`, v1
    `cpu.cfs_quota_us / cpu.cfs_period_us`). torch sizes its thread pool by the machine's core count; inside a container with a
    quota that over-subscribes the CPU leg (round 4: 128 threads on the GPU box's host ran the oracle 2.3x SLOWER than 8 threads
    of the 8-core build container)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = open(os.path.join(cgroup_root, "cpu.max")).read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = float(open(os.path.join(cgroup_root, "cpu", "cpu.cfs_quota_us")).read())
            per = float(open(os.path.join(cgroup_root, "cpu", "cpu.cfs_period_us")).read())
            if q > 0 and per > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    if quota is not None:
        n = min(n, max(1, int(quota + 0.5)))
    return max(1, n)


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(args) -> None:
    """`python bench.py --gpus N` outside a launcher: become `python -m torch.distributed.run ... bench.py <same flags>` (one
    process per GPU on this node, rendezvous on 127.0.0.1). stdout is inherited, so rank 0's JSON line is this process's."""
    port = os.environ.get("MASTER_PORT") or str(_free_port())
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    sys.stdout.flush()
    os.execv(sys.executable, cmd)


def broadcast_params(P, rank=None, world=None):
    """RCCL broadcast of rank 0's weights (paddlemix_amd/dist.py: 16-bit matrices on the wire, big tensors in place, small ones
    bucketed)."""
    from paddlemix_amd.dist import broadcast_params as _b
    return _b(P, src=0)


def main():
    args = parse()
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args)   # does not return
    world = int(os.environ.get("WORLD_SIZE", 1))
    # stdout carries ONE line, rank 0's JSON. The C libraries of the process write to fd 1 as well -- RCCL prints its version banner
    # there when the process ends, i.e. AFTER the JSON line (profiles/r04_s3_bench_force_dist_rccl_banner.txt, r05_s26_...) -- so fd 1
    # becomes stderr for everything except that line, which goes out through a duplicate of the original descriptor.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    if args.parity_child:
        args.no_cpu_baseline, args.no_roofline, args.no_parity_mode = True, True, True
        if not WORKLOADS[args.workload].get("sd3"):
            args.workload = "sdxl-1024-bs8"
    cpu = args.selftest_cpu
    if cpu:
        dev = torch.device("cpu")
        args.workload, args.no_cpu_baseline, args.no_roofline, args.no_parity_mode = "tiny-selftest", True, True, True
    else:
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    dist = None
    multi = world > 1 or args.force_dist     # the multi-rank code path (collectives included)
    if multi:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "RANK" not in os.environ:         # --force-dist outside a launcher: a one-rank group of its own
            os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
            os.environ.setdefault("MASTER_PORT", str(_free_port()))
        if cpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    def dev_sync():
        if not cpu:
            torch.cuda.synchronize()

    from paddlemix_amd import _lib
    _lib.set_elem_dtype(args.dtype)   # before anything loads the library
    from paddlemix_amd.schedulers import EulerDiscreteScheduler, FlowMatchEulerDiscreteScheduler
    from paddlemix_amd.unet import UNet2DConditionModel, synth_unet_params, unet_param_shapes
    is_sd3 = bool(WORKLOADS.get(args.workload, {}).get("sd3"))
    if is_sd3:
        from paddlemix_amd.sd3 import SD3Transformer2DModel as UNet2DConditionModel  # same program interface
        from paddlemix_amd.sd3 import sd3_param_shapes as unet_param_shapes, synth_sd3_params as synth_unet_params

    if cpu:
        from tests.configs import TINY
        WORKLOADS["tiny-selftest"] = dict(cfg=TINY, B=2, H=8, W=8, L=7, gflop_step=0.0)
    wl = WORKLOADS[args.workload]
    cfg, B, H, W, L = wl["cfg"], wl["B"], wl["H"], wl["W"], wl["L"]

    # ---- weights: rank 0 draws them, everyone else receives them over RCCL, as the 16-bit matrices the kernels consume ----
    from paddlemix_amd.dist import empty_wire_params, gather_latents, wire_params
    ed = _lib.elem_dtype()
    with_te = (args.text_encoders or multi) and not is_sd3 and args.workload.startswith("sdxl")
    te_cfgs = {}
    if with_te:
        from paddlemix_amd.clip import CLIPTextModel, CLIPTextModelWithProjection, clip_param_shapes, synth_clip_params
        te_cfgs = {"text_encoder": (CLIP_L, CLIPTextModel), "text_encoder_2": (CLIP_BIGG, CLIPTextModelWithProjection)}
    if args.parity_child:
        # the seeded CPU weights the committed oracle trajectory was computed with (exact in fp16 and bf16)
        from tests import parity_cases as PC
        pcase = PC.FWD_CASES["sd3_8x16x128x128_fwd"] if is_sd3 else PC.CASES[PARITY_CASES[0]]
        P = wire_params({k: v.to(dev) for k, v in PC.case_params(pcase).items()}, ed)
        PT = {}
    elif rank == 0:
        P = wire_params(synth_unet_params(cfg, seed=1234, device=dev), ed)
        PT = {k: wire_params(synth_clip_params(c, seed=77 + i, device=dev), ed) for i, (k, (c, _)) in enumerate(te_cfgs.items())}
    else:
        P = empty_wire_params(unet_param_shapes(cfg), ed, dev)
        PT = {k: empty_wire_params(clip_param_shapes(c), ed, dev) for k, (c, _) in te_cfgs.items()}
    bcast_s = bcast_bytes = None
    if multi:
        dev_sync()
        dist.barrier()
        t0 = time.time()
        bcast_bytes = broadcast_params(P) + sum(broadcast_params(v) for v in PT.values())
        dev_sync()
        bcast_s = time.time() - t0
    kw = {"weight_dtype": "fp8"} if wl.get("fp8") else {}
    if wl.get("a8"):
        kw["act_dtype"] = "fp8"
    if args.residual == "fp32":
        kw["residual_dtype"] = "fp32"
    if cpu:
        from tests.abi_emulator import on_emulator   # test plumbing only (see --selftest-cpu above)
        model = on_emulator(UNet2DConditionModel, cfg, P, device=dev, use_graph=not args.no_graph, **kw)
    else:
        model = UNet2DConditionModel(cfg, P, device=dev, use_graph=not args.no_graph, **kw)
    P_cpu_needed = rank == 0 and not multi and args.full and not args.no_cpu_baseline and not cpu
    if not P_cpu_needed:
        del P
    if not cpu:
        torch.cuda.empty_cache()

    # ---- synthetic inputs, resident in HBM ----
    g = torch.Generator(device=dev).manual_seed(rank)
    if is_sd3:
        sched = FlowMatchEulerDiscreteScheduler(shift=3.0)
        n_sched = 28
    else:
        sched = EulerDiscreteScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                       timestep_spacing="leading", steps_offset=1)
        n_sched = 30
    sched.set_timesteps(n_sched)
    latents = torch.randn(B, cfg["in_channels"] if is_sd3 else 4, H, W, generator=g, device=dev) * sched.init_noise_sigma
    enc = torch.randn(B, L, cfg["joint_attention_dim" if is_sd3 else "cross_attention_dim"], generator=g, device=dev)
    pooled = torch.randn(B, cfg["pooled_projection_dim"], generator=g, device=dev) if is_sd3 else None
    added = None
    if cfg.get("addition_embed_type") == "text_time":
        td = cfg["projection_class_embeddings_input_dim"] - 6 * cfg["addition_time_embed_dim"]
        added = dict(text_embeds=torch.randn(B, td, generator=g, device=dev),
                     time_ids=torch.tensor([[1024., 1024., 0., 0., 1024., 1024.]], device=dev).repeat(B, 1))
    te_s = None
    if with_te:
        # every rank encodes ITS prompts (synthetic token ids, its own seed) with the broadcast text encoders, once, outside the
        # timed region: encode_prompt of the SDXL pipeline (pipeline_stable_diffusion_xl.py:283-470) = hidden_states[-2] of both
        # encoders concatenated on the feature axis + the second encoder's pooled projection
        t0 = time.time()
        ids = torch.randint(3, 49000, (B, L), generator=g, device=dev)
        ids[:, 0], ids[:, -1] = 49406, 49407   # BOS ... EOS (the pooled row is the arg-max id's, modeling.py:470-480)
        te1 = te_cfgs["text_encoder"][1](CLIP_L, PT["text_encoder"], device=dev)
        te2 = te_cfgs["text_encoder_2"][1](CLIP_BIGG, PT["text_encoder_2"], device=dev)
        o1 = te1(ids, output_hidden_states=True)
        o2 = te2(ids, output_hidden_states=True)
        enc = torch.cat([o1.hidden_states[-2], o2.hidden_states[-2]], -1).float()
        added["text_embeds"] = o2.text_embeds.float()
        assert enc.shape == (B, L, cfg["cross_attention_dim"]) and added["text_embeds"].shape == (B, td)
        dev_sync()
        te_s = time.time() - t0
        del te1, te2, o1, o2, PT
        torch.cuda.empty_cache()
    plan = model._get_plan(B, H, W, L)
    if wl["gflop_step"] is None:
        wl = dict(wl, gflop_step=sum(fl for _, _, _, fl in plan.prog) / 1e9)
    # latent-update coefficients of every scheduler step, resident in HBM (no per-step host->device copy, so the host
    # can queue steps ahead of the GPU)
    if is_sd3:
        coef_host = [(1.0, float(sched.sigmas[k + 1] - sched.sigmas[k])) for k in range(n_sched)]
    else:
        coef_host = []
        for k in range(n_sched):
            sched._step_index = k
            coef_host.append(tuple(float(v) for v in sched.step_coefficients(sched.timesteps[k])))
        sched._step_index = None
    coef_all = torch.tensor(coef_host, device=dev, dtype=torch.float32).contiguous()
    lib = model._lib   # the loaded library (the C-ABI interpreter in the CPU self-test)
    stream = model._stream
    stream_ptr = model._stream_ptr
    lat0 = latents.clone()
    last = {}   # the noise prediction of the latest step (--dump-outputs)

    def step(i):
        """one denoising step, everything stream-ordered on the model's stream"""
        k = i % n_sched
        if k == 0:
            sched._step_index = None
            latents.copy_(lat0)
        t = sched.timesteps[k]
        if is_sd3:  # flow matching: x += (sigma_next - sigma) * v  (scheduling_flow_match_euler_discrete.py:244-278)
            model.stage_inputs(plan, latents, enc, pooled, float(t))
        else:
            sched._step_index = k
            scale = sched.model_input_scale(t)
            model.stage_inputs(plan, latents, float(t), enc, added, in_scale=scale)
        eps = last["noise_pred"] = model.run(plan)
        _lib.check(lib.mi355x_sd_axpby(latents.data_ptr(), eps.data_ptr(), latents.data_ptr(),
                                       coef_all.data_ptr() + 8 * k, latents.numel(), stream_ptr))

    def sync_all():
        dev_sync()
        if dist is not None:
            dist.barrier()
            dev_sync()

    # board clock / power WHILE the timed steps run (rank 0; one `rocm-smi` call from a helper thread ~0.4 s into the region: a host
    # process, nothing on the GPU): the step is power-managed (profiles/HISTORY.md section 5, round 4), so `value` is what the chip does at
    # THIS clock -- recorded next to it, never used in a formula. Absent tool / unparsable output: the field is null.
    board = {}

    def sample_board():
        import re
        import subprocess
        time.sleep(0.4)
        try:
            out = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=20).stdout
            sclk = re.findall(r"sclk clock level:[^(]*\((\d+)Mhz\)", out)
            power = re.findall(r"Power \(W\):\s*([\d.]+)", out)
            if sclk:
                board["sclk_mhz"] = int(sclk[local_rank if local_rank < len(sclk) else 0])
            if power:
                board["power_w"] = float(power[local_rank if local_rank < len(power) else 0])
        except Exception:
            pass

    sampler = None
    with (contextlib.nullcontext() if cpu else torch.cuda.stream(stream)):
        for i in range(args.warmup):
            step(i)
        sync_all()
        if rank == 0 and not cpu and args.full and args.steps >= 20:
            import threading
            sampler = threading.Thread(target=sample_board, daemon=True)
            sampler.start()
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(args.warmup + i)
        dev_sync()
        local_elapsed = time.perf_counter() - t0   # this rank's own K steps (reported per rank; not the metric)
        sync_all()
        elapsed = time.perf_counter() - t0         # the metric's clock: barrier + synchronize on both sides
    if not torch.isfinite(latents).all():
        raise SystemExit("non-finite latents")
    per_rank_ms = [1e3 * local_elapsed / args.steps]
    gathered_shape = None
    if dist is not None:
        tall = [torch.zeros(2, device=dev, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(tall, torch.tensor([elapsed, local_elapsed], device=dev, dtype=torch.float64))
        per_rank_ms = [1e3 * t[1].item() / args.steps for t in tall]
        elapsed = max(t[0].item() for t in tall)   # max over ranks
        allz = gather_latents(latents)      # the only other collective of the job: the ranks' results, once
        gathered_shape = list(allz.shape)
        if not torch.isfinite(allz).all():
            raise SystemExit("non-finite latents on some rank")
        if cpu and rank == 0:   # self-test: the ranks drew different prompts (per-rank seed) and the gather is rank-major
            assert torch.equal(allz[:B], latents) and (world == 1 or not torch.allclose(allz[:B], allz[B:2 * B]))
    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives from its last step: the updated latents (every rank's, rank-major, when the job
        # has several) and the model's noise prediction (rank 0's), float32. Before the roofline pass, which reuses the output buffer.
        # Above DUMP_BYTES in all (SD3 on 8 ranks: 72 MiB), every array keeps the same fixed, seeded, sorted sample of its batch rows.
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        outs = {"latents": allz if dist is not None else latents, "noise_pred": last["noise_pred"]}
        total = sum(4 * t.numel() for t in outs.values())
        for name, t in outs.items():
            if total > DUMP_BYTES:
                keep = max(1, t.shape[0] * DUMP_BYTES // total)
                rows = torch.randperm(t.shape[0], generator=torch.Generator().manual_seed(0))[:keep].sort().values
                t = t[rows.to(t.device)]
            np.save(os.path.join(args.dump_outputs, name + ".npy"), t.detach().float().cpu().numpy())

    res = {
        "metric": {"sdxl-1024-bs8": "UNet denoising steps/sec (SD-XL 1024^2, bs=8)",
                   "sd15-512-bs1": "UNet denoising steps/sec (SD-1.5 512^2, bs=1)",
                   "sd3-1024-bs8": "MMDiT denoising steps/sec (SD3-medium 1024^2, bs=8, bf16 weights)",
                   "sd3-1024-bs8-fp8w": "MMDiT denoising steps/sec (SD3-medium 1024^2, bs=8, fp8 weights)",
                   "sd3-1024-bs8-w8a8": "MMDiT denoising steps/sec (SD3-medium 1024^2, bs=8, fp8 weights + activations, fp8 MFMA)",
                   "tiny-selftest": "launcher self-test (no measurement)"}[args.workload],
        "value": world * args.steps / elapsed, "unit": "steps/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, **({"selftest": "CPU ranks + C-ABI interpreter on the tiny test UNet: launcher / rendezvous / timing "
                                              "protocol only, NOT a measurement"} if cpu else {}),
        "dtype": ("fp8 e4m3 (block GEMM operands) + " + args.dtype) if wl.get("a8") else args.dtype, "data": "synthetic",
        "config": {"workload": args.workload, "latents": [B, cfg["in_channels"] if is_sd3 else 4, H, W], "text": [B, L, cfg["joint_attention_dim" if is_sd3 else "cross_attention_dim"]],
                   "batch_per_gpu": B, "global_batch": B * world, "scheduler": "FlowMatchEuler/28" if is_sd3 else "EulerDiscrete/30",
                   "weights": f"random-init {args.dtype} (N(0,1/fan_in)), RCCL-broadcast from rank 0" if multi
                   else f"random-init {args.dtype} (N(0,1/fan_in))",
                   "parallelism": f"prompt-sharded dp{world}, no per-step collective", "hipgraph": bool(model.use_graph)},
        "tflops_effective": world * args.steps * wl["gflop_step"] / 1e3 / elapsed,
    }
    if sampler is not None:
        sampler.join(timeout=25)
        res["board_during_timed_region"] = dict(board, source="rocm-smi, one sample 0.4 s into the timed steps") if board else None
    if bcast_s is not None:
        res["weight_broadcast_s"] = bcast_s
        res["weight_broadcast_gb"] = bcast_bytes / 1e9
        res["per_rank_ms_per_step"] = [round(v, 3) for v in per_rank_ms]
        res["gathered_latents"] = gathered_shape
    if te_s is not None:
        res["text_encode_s"] = te_s
    res["config"]["residual_stream"] = args.residual
    if args.parity_child:
        # the SAME model object that was just timed replays the fixtures' loops (float64 latent state on the host)
        from tests import parity_cases as PC
        res["parity_live"] = {} if is_sd3 else {c: PC.device_report(c, model=model, dev=dev) for c in args.parity_cases.split(",") if c}
        # ... and ONE whole-batch forward at the launch set the metric times (SDXL 8x4x128x128: M = 8192 / 32768 GEMM tiles, no split-K;
        # SD3 8x16x128x128: 33 k-row tiles, 4,250-key joint attention, the fp8 modes against the oracle on the same quantised operands)
        # against the committed oracle forward of the same batch (tests/parity_cases.py FWD_CASES)
        fwd_name = "sdxl_8x4x128x128_fwd"
        if is_sd3:
            fwd_name = "sd3_8x16x128x128_fwd" + ("_w8a8" if wl.get("a8") else "_fp8w" if wl.get("fp8") else "")
        fw = PC.device_fwd_report(fwd_name, model, dev=dev)
        res["parity_live_bs8"] = dict({k: v for k, v in fw.items() if k != "pred"}, fixture=fwd_name)

    # ---- roofline of the dominant kernel: per-launch HIP-event timing on the launch stream, one eager step ----
    if rank == 0 and args.full and not args.no_roofline:
        model.profile = True
        model.kernel_times.clear()
        with torch.cuda.stream(stream):
            for i in range(2):
                model.kernel_times.clear()
                if is_sd3:
                    model.stage_inputs(plan, latents, enc, pooled, 500.0)
                else:
                    model.stage_inputs(plan, latents, 500.0, enc, added, in_scale=0.5)
                model._run_eager(plan)
        model.profile = False
        kinds, shapes = {}, {}
        for key, xs in model.kernel_times.items():
            kind = key.split(":")[0]
            k = kinds.setdefault(kind, dict(launches=0, ms=0.0, gflop=0.0))
            k["launches"] += len(xs)
            k["ms"] += 1e3 * sum(x[0] for x in xs)
            k["gflop"] += sum(x[1] for x in xs) / 1e9
            if ":" in key:
                shapes[key] = dict(n=len(xs), ms=round(1e3 * sum(x[0] for x in xs), 3),
                                   tflops=round(sum(x[1] for x in xs) / 1e12 / max(sum(x[0] for x in xs), 1e-12), 1))
        if os.environ.get("BENCH_SHAPES"):
            for key, v in sorted(shapes.items(), key=lambda kv: -kv[1]["ms"]):
                print(f"  {key:40s} n={v['n']:4d} {v['ms']:8.3f} ms {v['tflops']:8.1f} TFLOP/s", file=sys.stderr)
        total_ms = sum(v["ms"] for v in kinds.values())
        dom = max((k for k in kinds if kinds[k]["gflop"] > 0), key=lambda k: kinds[k]["ms"])
        d = kinds[dom]
        ach = d["gflop"] / d["ms"]  # GFLOP/ms == TFLOP/s
        names = {"gemm": "linear GEMM class: gemm_w4_kernel / gemm_pipe[_pre]_kernel<false,...> / gemm256_kernel<false> / gemm_small_kernel / gemm_bf16_kernel<false,...>",
                 "conv": "conv3x3 implicit-GEMM class: gemm_pipe_kernel<true,...> / gemm256_kernel<true>",
                 "attn": "attention16_kernel<LOG2> (16x16x32 MFMA; masks / head_dim != 64: attention_kernel<64,false>)"}
        # the W8A8 workload's GEMM class runs on the fp8 matrix pipe: price it against the fp8 peak
        peak = PEAK_FP8_TFLOPS if (wl.get("a8") and dom == "gemm") else PEAK_BF16_TFLOPS
        res["roofline"] = {"bound": "mfma", "kernel": names.get(dom, dom), "achieved": ach, "peak": peak,
                           "unit": "TFLOP/s", "frac": ach / peak, "traffic": None,
                           "launches_per_step": d["launches"], "avg_launch_ms": d["ms"] / d["launches"],
                           "algorithmic_gflop_per_step": d["gflop"]}
        # HBM traffic comes from rocprofv3 PMC passes (scripts/traffic.sh: FETCH_SIZE / WRITE_SIZE in separate passes,
        # gfx950 x2 read correction) -- it cannot be sampled from inside this process; the committed measurement of the
        # same workload is attached when present.
        import glob
        cands = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_traffic_{args.workload}.json")))
        tpath = cands[-1] if cands else os.path.join(ROOT, "profiles", f"r01_f_traffic_{args.workload}.json")
        if os.path.exists(tpath):
            tj = json.load(open(tpath))
            cls = tj["classes"].get(dom)
            if cls:
                res["roofline"]["traffic"] = cls["hbm_bytes_per_launch"]
                res["roofline"]["traffic_unit"] = "B/launch (class average; rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE)"
                res["roofline"]["traffic_source"] = os.path.relpath(tpath, ROOT)
        res["kernel_breakdown_ms"] = {k: round(v["ms"], 3) for k, v in sorted(kinds.items(), key=lambda kv: -kv[1]["ms"])}
        res["kernel_breakdown_tflops"] = {k: round(v["gflop"] / v["ms"], 1) for k, v in kinds.items() if v["gflop"] > 0}
        res["eager_step_ms_sum_of_kernels"] = total_ms

    # ---- CPU baseline: the torch-CPU oracle on a bounded sample of the same workload (rank 0, N=1 only) ----
    # ONE of the step's B prompts at the full latent geometry (exact attention cost; prompts are independent, so the step is
    # B such forwards), timed once after a small page-in call: ~10-30 s of CPU work. The full-batch measurement (2 timed
    # bs-B steps) is scripts/cpu_baseline.py -> profiles/r*_cpu_baseline_<workload>.json, attached when committed.
    if P_cpu_needed:
        threads = min(torch.get_num_threads(), usable_cpus())
        torch.set_num_threads(threads)   # (never more threads than the container's affinity mask / CPU quota grants)
        Pc = {k: v.float().cpu() for k, v in P.items()}
        del P
        gs = torch.Generator().manual_seed(0)
        # SDXL / SD3 (bs 8): ONE timed forward of one prompt; SD-1.5 (bs 1): BASELINE.md's "3 timed steps" of the whole (one-prompt) step
        n_fw = 3 if B == 1 else 1
        if is_sd3:
            from oracle.sd3_ref import sd3_forward
            s = torch.randn(1, cfg["in_channels"], H, W, generator=gs)
            e = torch.randn(1, L, cfg["joint_attention_dim"], generator=gs)
            pl = torch.randn(1, cfg["pooled_projection_dim"], generator=gs)
            # the oracle multiplies by the 16-bit weights as fp32 numbers: for the fp8 workloads this is the unquantised model (same FLOPs)
            fwd = lambda x: sd3_forward(Pc, cfg, x, e, pl, 500.0)   # noqa: E731
            page_in = s[:, :, :16, :16]
        else:
            from oracle import unet_ref as U
            s = torch.randn(1, 4, H, W, generator=gs)
            e = torch.randn(1, L, cfg["cross_attention_dim"], generator=gs)
            ad = None
            if added is not None:
                ad = dict(text_embeds=torch.randn(1, td, generator=gs), time_ids=added["time_ids"][:1].cpu())
            fwd = lambda x: U.unet_forward(Pc, cfg, x, 500, e, added_cond_kwargs=ad)   # noqa: E731
            page_in = s[:, :, :8, :8]
        with torch.no_grad():
            fwd(page_in)
            t0 = time.perf_counter()
            for _ in range(n_fw):
                fwd(s)
            cpu_s = (time.perf_counter() - t0) / n_fw
        what = "MMDiT" if is_sd3 else "UNet"
        res["cpu_baseline"] = {
            "value": 1.0 / (cpu_s * B), "unit": "steps/s", "cores": threads, "kind": "port",
            "sample": f"torch-CPU fp32 restatement of ppdiffusers (Paddle unavailable; plain-math attention as the reference's CPU path "
                      f"computes it, torch's CPU GEMMs underneath): {n_fw} {what} forward(s) of 1 of the step's {B} "
                      f"prompt(s) at the full {H}x{W} latents, {cpu_s:.2f} s each on {threads} threads; a step is {B} such forward(s) "
                      f"(prompts do not interact), value = 1 / ({B} x {cpu_s:.2f} s)",
        }
        import glob as _glob
        cb = sorted(_glob.glob(os.path.join(ROOT, "profiles", f"r*_cpu_baseline_{args.workload}.json")))
        if cb:
            res["cpu_baseline"]["full_batch_measured"] = dict(json.load(open(cb[-1])), source=os.path.relpath(cb[-1], ROOT))
    # ---- parity, measured by THIS run (child processes: the library is built per element type, one type per process; each child
    # builds the model from the fixtures' seeded weights, times the same step at the headline geometry and replays the full-depth
    # loops against the committed oracle trajectories) ----
    #   "parity":      the benchmarked mode itself (a short loop only: its throughput is the line's `value`)
    #   "parity_mode": the CHEAPEST mode that meets north_star's 1e-3 on the end latents -- fp16 elements with the same 16-bit
    #                  residual stream and the same kernels as the headline (the other instantiation of the element typedef)
    parity_legs = rank == 0 and not multi and not cpu and args.full and not args.no_parity_mode and not args.parity_child
    if parity_legs and args.workload == "sdxl-1024-bs8":
        import subprocess

        def parity_leg(dtype, residual, steps, warmup):
            t0 = time.time()
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--parity-child", "--dtype", dtype, "--residual", residual,
                                    "--steps", str(steps), "--warmup", str(warmup)], capture_output=True, text=True, timeout=900, cwd=ROOT,
                                   env={k: v for k, v in os.environ.items() if k not in ("MI355X_SD_DTYPE", "MI355X_SD_RESID")})
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
                if p.returncode != 0 or not line:
                    raise RuntimeError(p.stderr[-600:])
                c = json.loads(line[-1])
                live = c["parity_live"]
                return {"dtype": dtype, "residual": residual, "steps_per_s": c["value"], "ms_per_step": c["ms_per_step"], "steps": c["steps"],
                        "end_latents_rel_l2": {k: v["end_latents_rel"] for k, v in live.items()},
                        "pred_rel_l2_teacher_forced_max": {k: v["pred_rel_teacher_forced_max"] for k, v in live.items()},
                        # one forward of the whole 8x4x128x128 batch -- the launches the timed region replays -- vs the oracle's
                        "pred_rel_bs8": c.get("parity_live_bs8", {}).get("pred_rel_bs8"),
                        "pred_rel_bs8_per_prompt_max": c.get("parity_live_bs8", {}).get("pred_rel_bs8_per_prompt_max"),
                        "target_rel_l2": 1e-3, "meets_target": all(v["end_latents_rel"] < 1e-3 for v in live.values()),
                        "oracle": "committed trajectories of the torch-CPU restatement of ppdiffusers, reproduced bit for bit by the "
                                  "reference's own model code over a torch-backed paddle shim (tests/golden/parity; Paddle's kernels unpinned)",
                        "measured": "this run (child process, same box)", "seconds": round(time.time() - t0, 1)}
            except Exception as e:   # the headline number stands on its own; say why a leg is missing
                return {"dtype": dtype, "residual": residual, "error": str(e)[-600:]}

        res["parity"] = parity_leg(args.dtype, args.residual, 3, 1)
        if (args.dtype, args.residual) == ("fp16", "16"):
            res["parity_mode"] = dict(res["parity"], steps_per_s=res["value"], ms_per_step=res["ms_per_step"], steps=args.steps)
        else:
            res["parity_mode"] = parity_leg("fp16", "16", max(20, min(args.steps, 30)), 3)
        # Top level, not buried: does the mode `value` was measured in meet north_star's 1e-3 on the end latents -- and the throughput
        # of the cheapest mode that does (same kernels, fp16 elements). BASELINE.json names bf16 for this configuration, so `value`
        # stays the bf16 number and says so.
        res["meets_target"] = bool(res["parity"].get("meets_target", False))
        if res["parity_mode"].get("meets_target"):
            res["value_meeting_target"] = {"steps_per_s": res["parity_mode"]["steps_per_s"], "dtype": res["parity_mode"]["dtype"],
                                           "residual": res["parity_mode"]["residual"]}
    if parity_legs and is_sd3:
        # SD3 lines: one whole-batch forward of the benchmarked mode at the benchmarked geometry (8x16x128x128, 4,250-key joint
        # attention) against the committed oracle forward -- for the fp8 modes the oracle on the same quantised operands
        # (tests/parity_cases.py FWD_CASES; per-prediction bars of tests/test_gpu_parity_loops.py). A child process on the fixtures'
        # seeded weights; the end-latents target is asserted on the 28-step loop fixtures in the GPU suite, not here.
        import subprocess
        t0 = time.time()
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--parity-child", "--workload", args.workload, "--dtype", args.dtype,
                                "--steps", "3", "--warmup", "1"], capture_output=True, text=True, timeout=900, cwd=ROOT,
                               env={k: v for k, v in os.environ.items() if k not in ("MI355X_SD_DTYPE", "MI355X_SD_RESID")})
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not line:
                raise RuntimeError(p.stderr[-600:])
            c = json.loads(line[-1])["parity_live_bs8"]
            bar = {"sd3-1024-bs8": 1.6e-2 if args.dtype == "bf16" else 2.5e-3, "sd3-1024-bs8-fp8w": 1.6e-2, "sd3-1024-bs8-w8a8": 3.2e-2}[args.workload]
            res["parity"] = {"dtype": res["dtype"], "pred_rel_bs8": c["pred_rel_bs8"], "pred_rel_bs8_per_prompt_max": c["pred_rel_bs8_per_prompt_max"],
                             "fixture": c["fixture"], "bar_pred_rel": bar, "within_bar": c["pred_rel_bs8"] < bar,
                             "measured": "this run (child process, same box)", "seconds": round(time.time() - t0, 1)}
        except Exception as e:
            res["parity"] = {"error": str(e)[-600:]}
    if rank == 0:
        os.write(json_fd, (json.dumps(res) + "\n").encode())
    if dist is not None:
        dist.barrier()   # rank 0 ran the roofline pass meanwhile: tear the communicator down together
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
