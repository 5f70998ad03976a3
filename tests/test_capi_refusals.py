"""What the argument-checking entries of csrc/capi.hip answer before anything touches the device, as a table of literals: the GEMM-class
entries, the three attention entries and the seven base / `_ex` pairs share their bodies, and every refusal still carries the status
and the whole message of the entry that was called. The expected pairs were recorded from the library as it was before the bodies were
shared. Runs on a machine without a device only: the calls pass host addresses, which must never reach a launch."""
import pytest
import torch

from paddlemix_amd import _lib
from tests.header_decls import declared

INVALID, UNSUPPORTED = 1, 2
GEGLU, SILU, PAD_BR, CONV_KB64, SDPA_LOG2 = _lib.GEGLU, _lib.SILU, _lib.PAD_BR, _lib.CONV_KB64, _lib.SDPA_LOG2
PAIRS = ["adaln", "groupnorm_stats", "scale_shift_act", "layernorm", "fused_adaln_scale_residual", "conv_in3x3", "add_nchw"]
ENTRIES = (["linear", "linear_ex", "linear_ln", "linear_f8", "linear_f8_q", "conv3x3", "sdpa", "sdpa_ex", "sdpa_accum"] +
           [p + ex for p in PAIRS for ex in ("", "_ex")])
CONV = dict(B=1, Hs=4, Ws=4, Cin=8, Cout=8, stride=1, upsample=0, ws=None)   # a shape mi355x_sd_conv3x3 accepts

# (entry, the arguments that are not 0 / not the start of the host buffer, status, message); a pointer is given as its offset into the
# buffer in bytes, or None for NULL
LATER = [
    ("linear_f8", dict(flags=SILU), UNSUPPORTED, "mi355x_sd_linear_f8: only MI355X_SD_GELU_TANH is supported"),
    ("linear_f8_q", dict(flags=SILU), UNSUPPORTED, "mi355x_sd_linear_f8_q: only MI355X_SD_GELU_TANH is supported"),
    ("sdpa_ex", dict(flags=SDPA_LOG2, D=32, bias=None), UNSUPPORTED, "mi355x_sd_sdpa_ex: MI355X_SD_SDPA_LOG2 needs D == 64 and no mask"),
    ("sdpa_ex", dict(flags=SDPA_LOG2, D=64), UNSUPPORTED, "mi355x_sd_sdpa_ex: MI355X_SD_SDPA_LOG2 needs D == 64 and no mask"),
    ("sdpa_accum", dict(q=None, out_scale=0.0), INVALID, "mi355x_sd_sdpa_accum: null pointer"),
    ("adaln_ex", dict(mod_dtype=7), INVALID, "mi355x_sd_adaln_ex: mod_dtype must be MI355X_SD_MOD_F32 or MI355X_SD_MOD_ELEM"),
    ("fused_adaln_scale_residual_ex", dict(mod_dtype=7), INVALID,
     "mi355x_sd_fused_adaln_scale_residual_ex: mod_dtype must be MI355X_SD_MOD_F32 or MI355X_SD_MOD_ELEM"),
    ("conv3x3", dict(CONV, stride=3), INVALID, "mi355x_sd_conv3x3: bad shape"),
    ("conv3x3", dict(CONV, flags=GEGLU), UNSUPPORTED, "mi355x_sd_conv3x3: GEGLU epilogue is linear-only"),
    ("conv3x3", dict(CONV, flags=CONV_KB64), UNSUPPORTED, "mi355x_sd_conv3x3: MI355X_SD_CONV_KB64 needs Cin % 64 == 0"),
    ("conv3x3", dict(CONV, flags=PAD_BR), UNSUPPORTED, "mi355x_sd_conv3x3: MI355X_SD_PAD_BR is the stride-2 downsampler's padding"),
    ("conv3x3", dict(CONV, flags=PAD_BR, stride=2, Hs=1, Ws=1), INVALID, "mi355x_sd_conv3x3: image smaller than the padded 3 x 3 window"),
    ("linear", dict(ws=8, ws_bytes=64), INVALID, "mi355x_sd_linear: the workspace pointer must be 16-byte aligned"),
    ("linear_ex", dict(ws=8, ws_bytes=64), INVALID, "mi355x_sd_linear_ex: the workspace pointer must be 16-byte aligned"),
    ("linear_ln", dict(ws=8, ws_bytes=64), INVALID, "mi355x_sd_linear_ln: the workspace pointer must be 16-byte aligned"),
    ("conv3x3", dict(CONV, ws=8, ws_bytes=64), INVALID, "mi355x_sd_conv3x3: the workspace pointer must be 16-byte aligned"),
]


def answer(lib, entry, base, given):
    """(status, message) of mi355x_sd_<entry> with every integer and float 0 and every pointer `base` (NULL when base is None; the
    stream always NULL), except the arguments `given` names"""
    args = []
    for kind, name in declared()["mi355x_sd_" + entry][1]:
        pointer = kind.endswith("*")
        v = given.get(name, 0 if name != "stream" else None)
        args.append(v if not pointer else None if v is None or base is None else base + v)
    assert not set(given) - {n for _, n in declared()["mi355x_sd_" + entry][1]}, (entry, given)
    rc = getattr(lib, "mi355x_sd_" + entry)(*args)
    return rc, lib.mi355x_sd_last_error().decode()


no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="host addresses: with a device a call that is not refused would launch on them")


@no_device
@pytest.mark.parametrize("entry", ENTRIES)
def test_every_pointer_null_is_refused_under_the_entrys_own_name(entry):
    assert answer(_lib.load(), entry, None, {}) == (INVALID, f"mi355x_sd_{entry}: null pointer")


@no_device
@pytest.mark.parametrize("entry,given,status,message", LATER, ids=[f"{e}-{i}" for i, (e, *_) in enumerate(LATER)])
def test_later_refusals_keep_status_and_message(entry, given, status, message):
    buf = torch.full((4096,), 7.25)
    assert buf.data_ptr() % 16 == 0
    assert answer(_lib.load(), entry, buf.data_ptr(), given) == (status, message)
    assert bool((buf == 7.25).all())
