"""-m gpu: the row-map and layout kernels (csrc/misc.hip outside the direct convolutions, split_concat of csrc/fused_ops.hip) against
tests/rowmap_bounds.py: the bound class (silu, activation, gated_activation, softmax_rows, timestep_embedding, axpby, cfg_axpby,
latent_dist's sample) held to an elementwise float64 bound over the WHOLE output, the exact class (copy_rows, cast_rows, patchify,
unpatchify, split_concat, embed_tokens, add_nchw, mask_to_bias, latent_dist's moments) bit for bit against a torch restatement, on
coded inputs for the layout kernels. Every output sits in a canary buffer, every input gap holds NaN, every grid-stride loop takes
a second, ragged trip. The matrix lives in tests/rowmap_child.py and runs in a child process, once on the bf16 library and once
with MI355X_SD_DTYPE=fp16 (the bounds at fp16's u_out, where the activation bounds are tight enough to separate the GELU forms).
The children run one after another, each under its own time limit; one that dies of a signal or runs out of time ends the whole
pytest session with status 3 (tests/gpu_child.py). The wrappers' argument checks are tested here too: each refusal must raise
ValueError and leave a canary output untouched."""
import pytest
import torch

from tests.gpu_child import Family
from tests.rowmap_child import CASES

pytestmark = pytest.mark.gpu
FAMILY = {"silu": "activations", "act": "activations", "gated": "activations", "softmax": "softmax_rows", "temb": "timestep_embedding",
          "axpby": "axpby / cfg_axpby", "cfg": "axpby / cfg_axpby", "latent": "latent_dist"}


CHILD = Family("rowmap_child.py", "ROWMAP_JSON", None, timeout=300)


def _run(dtype):
    """every case's result on one build; a child runs once"""
    return CHILD.child((), {"MI355X_SD_DTYPE": dtype})   # (the production library of either element type: these launchers log no route)


def _check(name, v):
    assert "error" not in v, (name, v)
    assert v["rc"] == 0, (name, v)
    assert v["unwritten"] == 0, (name, v)       # every element of every output written
    assert v["overwritten"] == 0, (name, v)     # no row padding, nothing after the last row touched
    if "ratio" in v:
        assert v["ratio"] < 1.0, (name, v)
    for k in ("off", "wrapper_off", "pad_off"):   # bit equality: the restatement, the ops wrapper's compact call, the zero pad column
        if k in v:
            assert v[k] == 0, (name, k, v)
    assert "ratio" in v or "off" in v, (name, v)


@pytest.mark.parametrize("name", list(CASES))
def test_case_bf16(name):
    v = _run("bf16")[name]
    print(f"{name:<52} " + " ".join(f"{k} {v[k]:.3f}" if k == "ratio" else f"{k} {v[k]}" for k in v))
    _check(name, v)


@pytest.mark.parametrize("name", list(CASES))
def test_case_fp16(name):
    v = _run("fp16")[name]
    print(f"{name:<52} " + " ".join(f"{k} {v[k]:.3f}" if k == "ratio" else f"{k} {v[k]}" for k in v))
    _check(name, v)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_worst_err_bound_per_family(dtype):
    """(a report: what the bounds leave as headroom, per kernel family)"""
    got = _run(dtype)
    worst = {}
    for name, v in got.items():
        if "ratio" in v:
            f = FAMILY[CASES[name][0]]
            worst[f] = max(worst.get(f, 0.0), v["ratio"])
    print(dtype + ": " + "; ".join(f"{k} {w:.3f}" for k, w in sorted(worst.items())))
    assert all(w < 1.0 for w in worst.values()), worst


# ---- the wrappers refuse before any launch ----------------------------------------------------------------------------------------
CANARY_F = 7.25   # (exact in every dtype used below)


@pytest.fixture(scope="module")
def ops():
    from paddlemix_amd import ops as o
    o.init(0)
    return o


def _untouched(t):
    torch.cuda.synchronize()
    return bool((t == CANARY_F).all().item())


def test_axpby_refusals(ops):
    x, y = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda")
    c = torch.tensor([1.0, 2.0], device="cuda")
    out = torch.full((64,), CANARY_F, device="cuda")
    bad = [dict(x=x.double()), dict(y=y.half()), dict(x=x.cpu()), dict(y=y.cpu()), dict(c=c.cpu()), dict(c=c.double()), dict(c=c[:1]),
           dict(y=y[:32]), dict(y=torch.zeros(128, device="cuda")[::2]), dict(x=torch.zeros(128, device="cuda")[::2]),
           dict(out=torch.full((32,), CANARY_F, device="cuda")), dict(out=torch.full((64,), CANARY_F, device="cuda", dtype=torch.float64)),
           dict(out=torch.full((128,), CANARY_F, device="cuda")[::2]), dict(out=torch.full((64,), CANARY_F))]
    for kw in bad:
        a = dict(x=x, y=y, c=c, out=out)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.axpby(a["x"], a["y"], a["c"], a["out"])
        assert _untouched(a["out"]) and _untouched(out), kw
    assert torch.equal(ops.axpby(x + 1, y + 1, c, out), torch.full((64,), 3.0, device="cuda"))   # (and the good call writes)


def test_patchify_unpatchify_refusals(ops):
    from paddlemix_amd import _lib
    ed = _lib.elem_dtype()
    x = torch.zeros(2, 3, 8, 12, device="cuda")
    for bad in (x.double(), x.cpu(), x.permute(0, 1, 3, 2), x[:, :, :, ::2], x[0]):
        with pytest.raises(ValueError):
            ops.patchify(bad, 2)
    with pytest.raises(ValueError):
        ops.patchify(x, 5)
    rows = torch.full((2 * 4 * 6, 2 * 2 * 3), CANARY_F, device="cuda", dtype=ed)
    for args in ((rows[:-1], 2, 3, 8, 12, 2), (rows[:, :-1], 2, 3, 8, 12, 2), (rows, 2, 3, 8, 12, 4), (rows, 2, 4, 8, 12, 2),
                 (rows, 3, 3, 8, 12, 2), (rows, 2, 3, 8, 14, 2), (rows.float(), 2, 3, 8, 12, 2), (rows.cpu(), 2, 3, 8, 12, 2),
                 (rows.t().contiguous().t(), 2, 3, 8, 12, 2), (rows, 2, 3, 9, 12, 2)):
        with pytest.raises(ValueError):
            ops.unpatchify(*args)
    assert ops.unpatchify(rows, 2, 3, 8, 12, 2).shape == (2, 3, 8, 12)


def test_softmax_out_refusals(ops):
    from paddlemix_amd import _lib
    ed = _lib.elem_dtype()
    x = torch.zeros(3, 8, device="cuda")
    for out in (torch.full((3, 4), CANARY_F, device="cuda", dtype=ed), torch.full((4, 8), CANARY_F, device="cuda", dtype=ed),
                torch.full((3, 8), CANARY_F, device="cuda"), torch.full((3, 8), CANARY_F, dtype=ed),
                torch.full((3, 16), CANARY_F, device="cuda", dtype=ed)[:, ::2], torch.full((24,), CANARY_F, device="cuda", dtype=ed)):
        with pytest.raises(ValueError):
            ops.softmax_rows(x, out=out)
        assert _untouched(out)
    wide = torch.full((3, 16), CANARY_F, device="cuda", dtype=ed)
    ops.softmax_rows(x, out=wide[:, :8])
    assert _untouched(wide[:, 8:]) and bool((wide[:, :8] == 0.125).all().item())


def test_gated_activation_and_embed_refusals(ops):
    from paddlemix_amd import _lib
    ed = _lib.elem_dtype()
    with pytest.raises(ValueError):
        ops.gated_activation(torch.zeros(4, 15, device="cuda", dtype=ed))
    with pytest.raises(ValueError):
        ops.gated_activation(torch.zeros(4, 16, dtype=ed))
    with pytest.raises(ValueError):
        ops.gated_activation(torch.zeros(4, 16, device="cuda"))
    ids = torch.tensor([0, 3, 9], dtype=torch.int32, device="cuda")
    tok, pos = torch.zeros(10, 16, device="cuda", dtype=ed), torch.zeros(4, 16, device="cuda", dtype=ed)
    for t, p in ((tok.float(), pos), (tok, pos.float()), (tok.cpu(), pos), (tok, pos.cpu()), (tok, pos[:, :8].contiguous()),
                 (torch.zeros(10, 32, device="cuda", dtype=ed)[:, ::2], pos), (tok, torch.zeros(4, 32, device="cuda", dtype=ed)[:, :16]),
                 (tok.reshape(-1), pos)):
        with pytest.raises(ValueError):
            ops.embed_tokens(ids, t, p, 3)
    assert ops.embed_tokens(ids, tok, pos, 3).shape == (3, 16)
