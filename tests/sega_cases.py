"""The cases of the semantic-guidance tests (tests/test_sega_host.py, tests/sega_child.py, tests/test_gpu_sega.py,
scripts/make_sega_golden.py) -- TEST INFRASTRUCTURE ONLY: the kernel matrix of mi355x_sd_sega_guidance, the closed-form stand-in
U-Net and the settings of the recorded loops."""
import numpy as np
import torch

from paddlemix_amd import schedulers as S
from paddlemix_amd import sega_forms as SF

GS = 7.5
SCHED = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SCHEDULERS = {"euler": lambda: S.EulerDiscreteScheduler(**SCHED),
              "ddim": lambda: S.DDIMScheduler(clip_sample=False, set_alpha_to_one=False, steps_offset=1, **SCHED),
              "dpm": lambda: S.DPMSolverMultistepScheduler(**SCHED), "heun": lambda: S.HeunDiscreteScheduler(**SCHED)}

# ------------------------------------------------------------------------------------------------- the kernel matrix
# The kernel has ONE form for every plane size (keys recomputed per digit pass, a 1024-thread block per plane) and two load paths in
# the selection: 16-byte vectors (hw % 4 == 0, eps aligned) and element by element. The sizes: 1, 2 (hi == the last element), 5 (an
# integral rank at q = 0.5), both sides of a wave (63, 64, 65), 99, the block (1024: one element per thread; 4099: odd, more than
# one trip), 16384 (the SDXL latent) and the cap 65536.
QS = (0.0, 0.75, 0.9, 0.995, 1.0)
CONTENTS = ("ties", "zero", "negzero", "inf", "nan", "offset50")
FORMS = ("all", "partial", "none", "cooled_reversed", "mom0_extra")


def step_form(name, n):
    """-> (i, kwargs of sega_forms.rows) that puts step i in the named form, for n concepts"""
    lst = lambda *v: list(v[:n])   # noqa: E731
    base = dict(guidance_scale=GS, edit_momentum_scale=0.3, edit_mom_beta=0.4, edit_guidance_scale=lst(5.0, 4.0, 6.5),
                reverse_editing_direction=lst(False, True, False), edit_warmup_steps=lst(0, 0, 0), edit_cooldown_steps=None,
                edit_weights=lst(1.0, 0.5, 2.0))
    if name == "partial":
        base.update(edit_warmup_steps=lst(0, 5, 0))        # n == 1 has no partial regime: it is "all" then
    elif name == "none":
        base.update(edit_warmup_steps=lst(5, 5, 5))
    elif name == "cooled_reversed":
        base.update(edit_cooldown_steps=lst(1, 9, 9), reverse_editing_direction=lst(True, True, False))
    elif name == "mom0_extra":
        base.update(edit_momentum_scale=0.0)
    return 2, base


def _case(hw, n, batch, q, content="ties", form="all", off=0, extra=None):
    return dict(hw=hw, n=n, batch=batch, channels=4, q=q, content=content, form=form, off=off,
                extra=(form == "mom0_extra") if extra is None else extra)


KERNEL = {}
for _hw in (1, 2, 5, 63, 64, 65, 99, 1024, 4099, 16384):
    for _k, _q in enumerate(QS):
        _n, _b = (1, 2, 3)[(_k + _hw) % 3], (1, 3)[(_k + _hw) % 2]
        if _hw >= 4099:
            _b = 1
        KERNEL[f"hw{_hw} q{_q} n{_n} b{_b}"] = _case(_hw, _n, _b, _q, content=("ties", "offset50")[_k % 2], form=FORMS[_k % len(FORMS)])
KERNEL["hw5 q0.5 integral rank"] = _case(5, 2, 3, 0.5)
KERNEL["hw65536 q0.9"] = _case(65536, 2, 1, 0.9, content="offset50")
KERNEL["hw1024 q0.9 off4"] = _case(1024, 2, 3, 0.9, off=1, extra=True)
for _c in CONTENTS:
    KERNEL[f"hw99 q0.75 {_c}"] = _case(99, 2, 3, 0.75, content=_c)
    KERNEL[f"hw1024 q0.9 {_c}"] = _case(1024, 3, 1, 0.9, content=_c, form="partial")
for _f in FORMS:
    KERNEL[f"hw64 q0.9 n3 {_f}"] = _case(64, 3, 3, 0.9, form=_f)
    KERNEL[f"hw65 q0.75 n2 {_f} extra"] = _case(65, 2, 1, 0.75, form=_f, extra=True)


def kernel_inputs(spec, seed):
    """-> (eps [2 + n, B, C, hw], momentum [B, C, hw], extra or None, row words int32): fp32 CPU. Every concept of a case shares the
    case's threshold q. "ties": every value a multiple of 0.25 in +- pairs, so |g| has heavy ties across lo / hi and every product
    with the scales (5, 4, 6.5) is exact; "offset50": a common offset of 50 on every group (it cancels in e - u, at 50's ulp)."""
    hw, n, B, C, content = spec["hw"], spec["n"], spec["batch"], spec["channels"], spec["content"]
    g = torch.Generator().manual_seed(seed)
    shape = (2 + n, B, C, hw)
    if content == "offset50":
        eps = 50.0 + torch.randn(shape, generator=g)
    else:
        eps = torch.randint(-12, 13, shape, generator=g).float() * 0.25
        d, half = torch.randint(-12, 13, (n, B, C, hw), generator=g).float() * 0.25, hw // 2
        d[..., half:2 * half] = -d[..., :half]                           # e - u at i + half is -(e - u) at i: +- pairs of g
        eps[2:] = eps[:1] + d                                            # (exact: small multiples of 0.25)
    if content == "zero":
        eps[2:] = eps[:1]                                                # g == 0 everywhere: thr = 0, everything passes
    elif content == "negzero":
        eps[2:, :, :, ::2] = eps[:1, :, :, ::2]                          # zeros of g ...
        eps[0, :, :, ::4] = 0.0
        eps[2:, :, :, ::4] = -0.0                                        # ... and (-0.0 - 0.0) * s = -0.0 or +0.0 by the scale's sign
    elif content == "inf":
        eps[2, :, :, 0] = float("inf")
        eps[2, 0, 1, -1] = float("-inf")
    elif content == "nan":
        eps[2, 0, 1, hw // 3] = float("nan")                             # one NaN, one plane of concept 0
    momentum = torch.randint(-8, 9, (B, C, hw), generator=g).float() * 0.125 if content != "offset50" else torch.randn((B, C, hw), generator=g)
    extra = torch.randn((B, C, hw), generator=g) if spec["extra"] else None
    i, kw = step_form(spec["form"], n)
    table = SF.rows(i + 1, n, hw, edit_threshold=spec["q"], **kw)
    return eps, momentum, extra, torch.from_numpy(table[i].view(np.int32).copy())


# ------------------------------------------------------------------------------------------------- the loops
class FormulaUNet:
    """eps = 0.6 tanh(x) cos(t / 300) + 0.3 sin(3 x + 5 m) + 0.05 m, m the mean of the sample's text tokens: nonlinear in the
    latents and in m, so the concepts differ per element and the mask matters. fp32, on whatever the loop feeds it."""
    dtype = torch.float32

    def __init__(self, config):
        self.config = config

    def __call__(self, x, t, encoder_hidden_states=None, return_dict=False, **kw):
        c = torch.cos(torch.as_tensor(float(t), dtype=torch.float32) / 300.0)
        m = encoder_hidden_states.mean(dim=(1, 2))[:, None, None, None]
        return (0.6 * torch.tanh(x) * c + 0.3 * torch.sin(3.0 * x + 5.0 * m) + 0.05 * m,)


STEPS, BATCH, HW, TOKENS, DIM = 5, 2, 8, 7, 32
GOLDEN_SEED = 33
PROMPTS, NEGATIVE, CONCEPTS = ["p0", "p1"], ["", ""], ["c0", "c1"]
VOCAB = {"p0": 0, "p1": 1, "": 2, "c0": 3, "c1": 4}


def embedding_table():
    """[len(VOCAB), TOKENS, DIM]: what the stand-in text encoder of the recorder returns for a prompt string; the concepts' rows are
    spread so that their means differ by a few tenths"""
    g = torch.Generator().manual_seed(GOLDEN_SEED)
    table = torch.randn(len(VOCAB), TOKENS, DIM, generator=g)
    return table + torch.tensor([0.0, 0.1, -0.1, 0.4, -0.3])[:, None, None]


def loop_inputs(n):
    """(prompt_embeds [B, T, D], negative [B, T, D], edit [n, B, T, D] concept-major, initial noise, sem_guidance [2 STEPS, ...])"""
    table = embedding_table()
    pick = lambda names: table[[VOCAB[k] for k in names]]   # noqa: E731
    g = torch.Generator().manual_seed(GOLDEN_SEED + 1)
    lat = torch.randn(BATCH, 4, HW, HW, generator=g)
    sem = 0.05 * torch.randn(2 * STEPS, BATCH, 4, HW, HW, generator=g)
    edit = torch.stack([pick([c] * BATCH) for c in CONCEPTS[:n]])
    return pick(PROMPTS), pick(NEGATIVE), edit, lat, sem


_TWO = dict(reverse_editing_direction=[False, True], edit_guidance_scale=[5.0, 4.0], edit_warmup_steps=[0, 2], edit_cooldown_steps=[3, 5],
            edit_threshold=[0.9, 0.75], edit_weights=[1.0, 0.5], edit_momentum_scale=0.3, edit_mom_beta=0.4)
# Heun runs 2 * steps - 1 iterations and the reference's per-step bookkeeping (``uncond_estimates`` ...: steps + 1 rows, REF :550) overflows
# past steps == 2, so its own pipeline cannot run a longer Heun loop: that loop is recorded at 2 steps (3 iterations: partial, partial
# all warm with concept 0 cooled down), every other loop at STEPS.
GOLDEN_STEPS = {"heun_two_lists": 2}
GOLDEN = {   # name: (scheduler, concepts, uses sem_guidance, the edit arguments)
    "ddim_two_lists": ("ddim", 2, False, _TWO),
    "euler_two_lists_sem_mom0": ("euler", 2, True, dict(_TWO, edit_momentum_scale=0.0)),
    "dpm_one_scalars": ("dpm", 1, False, dict(edit_guidance_scale=5, edit_warmup_steps=2, edit_threshold=0.9)),
    "heun_two_lists": ("heun", 2, False, dict(_TWO, edit_cooldown_steps=[2, 5], edit_weights=[2.0, 1.0], edit_mom_beta=0.6)),
    "ddim_one_reversed": ("ddim", 1, False, dict(reverse_editing_direction=True, edit_guidance_scale=6.0, edit_warmup_steps=0,
                                                 edit_cooldown_steps=3, edit_threshold=0.75, edit_momentum_scale=0.0)),
    "euler_two_scalars": ("euler", 2, False, dict(edit_guidance_scale=4.0, edit_warmup_steps=2, edit_threshold=0.9,
                                                  edit_momentum_scale=0.3, edit_mom_beta=0.4)),
    "dpm_two_lists_sem_negative_weight": ("dpm", 2, True, dict(_TWO, edit_weights=[1.0, -1.0])),
}
