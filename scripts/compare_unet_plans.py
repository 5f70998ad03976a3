#!/usr/bin/env python
"""The C++ U-Net planner and weight packer of one checkout, written out as text, so that two checkouts can be compared by `diff`.

    git worktree add /tmp/old <commit>
    python scripts/compare_unet_plans.py /tmp/old/paddlemix_amd/csrc /tmp/dump_old
    python scripts/compare_unet_plans.py paddlemix_amd/csrc /tmp/dump_new
    diff -r /tmp/dump_old /tmp/dump_new && wc -l /tmp/dump_new/*

Builds scripts/c/unet_plan_dump.cpp against the given csrc directory (host code only; no GPU is touched) and runs it over: the 15
configs of tests/test_cexec_host_logic.py at (2, 16, 16, 7) with the 16-bit and the fp32 residual stream; every combination of the
mi355x_sd_unet_plan_ex flags on TINY, MINI_XL and two one-level models whose attention runs at full resolution (the only ones a
self-attention mask fits; head_dim 8 and 64); MINI_XL at the odd sizes; SDXL at (2, 128, 128, 77); TINY, MINI_XL and SDXL with FreeU
on (a seventh field, with and without ControlNet residuals and the fp32 residual stream). One file per config: every packed
tensor's place, every buffer, every launch with every argument; `images.sha256` holds the hash of every packed weight image."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from tests.configs import MINI_XL, SD15, SDXL, TINY   # noqa: E402
from tests.test_cexec_host_logic import CLASS_CONFIGS   # noqa: E402

ONE_LEVEL = dict(TINY, block_out_channels=(64,), down_block_types=("CrossAttnDownBlock2D",), up_block_types=("CrossAttnUpBlock2D",))
BOTH = ["2,16,16,7,0,0", "2,16,16,7,0,1"]
FLAGS = [f"2,16,16,7,{f},{r}" for f in range(8) for r in (0, 1)]
CASES = {"tiny": (TINY, FLAGS), "mini-xl": (MINI_XL, FLAGS + ["1,18,18,77,0,0", "1,20,10,77,0,0", "1,9,14,77,0,0", "1,18,18,77,4,1"]),
         "sd15": (SD15, BOTH), "sdxl": (SDXL, BOTH + ["2,128,128,77,0,0"]),
         "one-level": (ONE_LEVEL, FLAGS), "one-level-hd64": (dict(ONE_LEVEL, attention_head_dim=1), FLAGS)}
CASES.update({k: (v, BOTH) for k, v in CLASS_CONFIGS.items()})
FREEU = ["2,16,16,7,0,0,1", "2,16,16,7,0,1,1", "2,16,16,7,4,0,1", "1,18,18,77,0,0,1"]   # (the files of a checkout without FreeU differ here only)
CASES.update({"tiny-freeu": (TINY, FREEU[:3]), "mini-xl-freeu": (MINI_XL, FREEU), "sdxl-freeu": (SDXL, FREEU[:2])})


def main(csrc, out):
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "unet_plan_dump")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-w", "-I", csrc,
                    os.path.join(ROOT, "scripts", "c", "unet_plan_dump.cpp"), "-o", exe], check=True)
    with open(os.path.join(out, "images.sha256"), "w") as sums:
        for name, (cfg, plans) in CASES.items():
            cj, img = os.path.join(out, "config.json"), os.path.join(out, "image.bin")
            with open(cj, "w") as f:
                json.dump(cfg, f)
            with open(os.path.join(out, name + ".txt"), "w") as f:
                subprocess.run([exe, cj, img] + plans, stdout=f, check=True)
            h = hashlib.sha256()
            with open(img, "rb") as f:
                for chunk in iter(lambda: f.read(1 << 24), b""):
                    h.update(chunk)
            sums.write(f"{h.hexdigest()}  {name}\n")
            os.remove(img)
            os.remove(cj)
    os.remove(exe)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2]))
