"""Shared host machinery of the MI355X models: symbolic addresses, row views, and the static program of C-ABI
launches (eager run with optional per-launch HIP-event timing, hipGraph capture / replay on the model's stream)."""
from __future__ import annotations

import contextlib
import contextvars

import ctypes
from typing import Callable, Dict, List, Optional

import torch

from . import _lib
from ._lib import CONV_KB64, GEGLU, OUT_F32, PAD_BR, R_F32

WORKSPACE_BYTES = 32 << 20   # split-K partial sums (the planner shrinks the split count to fit) AND the just-in-time widened copy of a
                             # weight-only-fp8 matrix (2 * N * K bytes, <= ~19 MB for SD3-medium): the `ws, ws_bytes` arguments of the
                             # GEMM-class entry points (include/mi355x_sd.h, ABI 12)


class _Ref:
    """Symbolic device address inside a named scratch buffer (resolved after all sizes are known)."""
    __slots__ = ("buf", "off")

    def __init__(self, buf: str, off: int = 0):
        self.buf, self.off = buf, off

    def __add__(self, nbytes: int) -> "_Ref":
        return _Ref(self.buf, self.off + nbytes)


class _V:
    """Row view: `rows` rows of `C` channels of `es` bytes each (2 = the build's 16-bit element, 4 = fp32: the residual
    stream of the fp32-residual mode), row stride `ld` elements, at address `p` (int or _Ref)."""
    __slots__ = ("p", "rows", "C", "ld", "es")

    def __init__(self, p, rows, C, ld=None, es=2):
        self.p, self.rows, self.C, self.ld, self.es = p, rows, C, (C if ld is None else ld), es

    def cols(self, off: int, C: int) -> "_V":
        return _V(self.p + self.es * off, self.rows, C, self.ld, self.es)

    @classmethod
    def of(cls, t: torch.Tensor) -> "_V":
        """the rows of a 2-D tensor"""
        return cls(t.data_ptr(), t.shape[0], t.shape[1], t.stride(0), t.element_size())


class _Plan:
    pass


class PlanBuilder:
    """What a model's ``_build_plan`` writes its launch plan with: the new ``plan``, the buffers it will own, and one method per launch
    form that two or more model families emit (a form only one family emits is a local function over ``emit`` next to that family).
    ``B`` is the batch every batched launch of the plan runs over."""

    def __init__(self, model: "DeviceProgram", B: int):
        self.model, self.B = model, B
        self.lib, self.W, self.device = model._lib, model.w, model.device
        self.stream, self.gemm_ws = model._stream_ptr, model._gemm_ws
        self.plan = _Plan()
        self.prog: List[tuple] = []          # (cfunc, args (list with _Ref placeholders), kind, flops)
        self.scratch: Dict[str, int] = {}
        self.keep: List[torch.Tensor] = []

    def sc(self, name: str, nbytes: int) -> _Ref:
        """the named scratch buffer, at least ``nbytes`` large (one buffer per name, sized by its largest request)"""
        self.scratch[name] = max(self.scratch.get(name, 0), nbytes)
        return _Ref(name)

    def persist(self, shape, dtype) -> torch.Tensor:
        t = torch.empty(shape, device=self.device, dtype=dtype)
        self.keep.append(t)
        return t

    def wp(self, key: str) -> int:
        return self.W[key].data_ptr()

    def emit(self, fn, args, kind, flops=0.0, desc="") -> None:
        self.prog.append((fn, list(args), kind if not desc else f"{kind}:{desc}", flops))

    def finish(self) -> _Plan:
        """allocate the scratch buffers (after everything persisted so far), resolve every _Ref, hand the plan over"""
        base = {n: self.persist((max(nb, 16),), torch.uint8).data_ptr() for n, nb in self.scratch.items()}
        plan = self.plan
        plan.prog = [(fn, tuple(base[a.buf] + a.off if isinstance(a, _Ref) else a for a in args), kind, fl)
                     for fn, args, kind, fl in self.prog]
        plan.keep, plan.graph = self.keep, None
        return plan

    # ---- launch forms shared by two or more families (`ws, ws_bytes` of the GEMM-class calls: ABI 12) ----
    def linear(self, a: _V, w, out: _V, bias=True, R: Optional[_V] = None, flags=0, out_scale=1.0, rowbias=None, rpb=0, ld_rb=0,
               bkey=None, desc=None) -> None:
        """out = (a W^T + bias + row bias) * out_scale + R with the epilogue ``flags``. ``w``: a weight key (matrix ``w.w``, bias ``w.b``
        or ``bkey``) or, for activations times activations, the _V of the [N, K] operand (``bias=False``)."""
        if isinstance(w, _V):
            assert not bias and w.ld == w.C, "an activation operand is dense and has no bias"
            wptr, N, K = w.p, w.rows, w.C
        else:
            (N, K), wptr = self.W[w + ".w"].shape, self.wp(w + ".w")
        assert K == a.C, (w, K, a.C)
        assert a.es == 2, (w, "fp32 rows cannot be an MFMA operand")
        flags |= (OUT_F32 if out.es == 4 else 0) | (R_F32 if (R is not None and R.es == 4) else 0)
        self.emit(self.lib.mi355x_sd_linear,
                  (a.p, a.ld, wptr, out.p, out.ld, a.rows, N, K, self.wp(bkey or w + ".b") if bias else None, rowbias, rpb, ld_rb,
                   R.p if R else None, R.ld if R else 0, out_scale, flags, *self.gemm_ws, self.stream), "gemm", 2.0 * a.rows * N * K,
                  f"{a.rows}x{N}x{K}" + ("g" if flags & GEGLU else "") if desc is None else desc)

    def linear_ex(self, a: _V, wkey: str, out: _V, *, flags=0, R: Optional[_V] = None, gate=None, ld_gate=0, rpb=0, a_rpb=0, a_bs=0,
                  c_rpb=0, c_bs=0, bias=True) -> None:
        """mi355x_sd_linear_ex: ``linear`` with a row remap of A (a_rpb rows per batch, batch stride a_bs) and of C, a per-row-block
        ``gate`` (row stride ld_gate, rpb rows per batch) on the product, and the weight's per-channel scale ``wkey.s`` if it has one"""
        w = self.W[wkey + ".w"]
        N, K = w.shape
        assert K == a.C, (wkey, K, a.C)
        ws = self.W.get(wkey + ".s")
        self.emit(self.lib.mi355x_sd_linear_ex,
                  (a.p, a.ld, a_rpb, a_bs, w.data_ptr(), ws.data_ptr() if ws is not None else None, out.p, out.ld, c_rpb, c_bs,
                   a.rows, N, K, self.wp(wkey + ".b") if bias else None, None, 0, gate, ld_gate if gate is not None else 0, rpb,
                   R.p if R else None, R.ld if R else 0, 1.0, flags, *self.gemm_ws, self.stream), "gemm", 2.0 * a.rows * N * K,
                  f"{a.rows}x{N}x{K}")

    def conv3(self, x: _V, h, w_, wkey, out: _V, stride=1, up=0, rowbias=None, ld_rb=0, R: Optional[_V] = None, out_scale=1.0,
              flags=0) -> None:
        """3x3 conv of B images of h x w (x2 nearest upsampling folded in with ``up``); MI355X_SD_PAD_BR in ``flags`` pads bottom / right
        only (one zero row and column instead of two)"""
        B, w = self.B, self.W[wkey + ".w"]
        Cout = w.shape[0]
        pad2 = 1 if flags & PAD_BR else 2
        ho, wo = ((h << up) + pad2 - 3) // stride + 1, ((w_ << up) + pad2 - 3) // stride + 1
        assert x.es == 2, (wkey, "fp32 rows cannot be an MFMA operand")
        flags |= (OUT_F32 if out.es == 4 else 0) | (R_F32 if (R is not None and R.es == 4) else 0)
        flags |= CONV_KB64 if wkey in getattr(self.model, "_kb64", ()) else 0
        self.emit(self.lib.mi355x_sd_conv3x3,
                  (x.p, x.ld, B, h, w_, x.C, stride, up, w.data_ptr(), out.p, out.ld, Cout, self.wp(wkey + ".b"), rowbias,
                   ld_rb if rowbias is not None else 0, R.p if R else None, R.ld if R else 0, out_scale, flags, *self.gemm_ws,
                   self.stream), "conv", 2.0 * B * ho * wo * Cout * 9 * x.C,
                  f"{B * ho * wo}x{Cout}x{9 * x.C}" + ("s2" if stride == 2 else "") + ("up" if up else ""))

    def gnorm(self, x: _V, hw, nkey, eps, silu, raw16: Optional[_V] = None) -> _V:
        """GroupNorm (+SiLU) of x -> 16-bit rows. fp32-residual mode: x is fp32; `raw16` (optional) receives the 16-bit
        rounding of the raw x rows in the same pass (the operand of a conv_shortcut GEMM)."""
        lib, sc, emit, wp, B, stream = self.lib, self.sc, self.emit, self.wp, self.B, self.stream
        groups = self.model.cfg["norm_num_groups"]
        ws = sc("gn_ws", 4 * lib.mi355x_sd_groupnorm_workspace_floats(B, hw, x.C))
        ss = sc("gn_ss", 4 * B * 2 * x.C)
        y = _V(sc("gn", 2 * x.rows * x.C), x.rows, x.C)
        silu = 1 if silu else 0
        if x.es == 2 and lib.mi355x_sd_groupnorm_act_fits(hw, x.C, groups):
            # small (batch, group) chunks: statistics + affine (+SiLU) in one launch (csrc/norm.hip gn_fused_kernel)
            assert raw16 is None
            emit(lib.mi355x_sd_groupnorm_act, (x.p, B, hw, x.C, x.ld, groups, eps, wp(nkey + ".g"), wp(nkey + ".b"), silu, y.p, y.ld,
                                               stream), "gn_fused")
        elif x.es == 2:
            assert raw16 is None
            emit(lib.mi355x_sd_groupnorm_stats, (x.p, B, hw, x.C, x.ld, groups, eps, wp(nkey + ".g"), wp(nkey + ".b"), ws, ss, stream),
                 "gn_stats")
            emit(lib.mi355x_sd_scale_shift_act, (x.p, B, hw, x.C, x.ld, ss, silu, y.p, y.ld, stream), "gn_apply")
        else:
            emit(lib.mi355x_sd_groupnorm_stats_ex, (x.p, B, hw, x.C, x.ld, groups, eps, wp(nkey + ".g"), wp(nkey + ".b"), ws, ss, 1,
                                                    stream), "gn_stats")
            emit(lib.mi355x_sd_scale_shift_act_ex, (x.p, B, hw, x.C, x.ld, ss, silu, y.p, y.ld, 1, raw16.p if raw16 else None,
                                                    raw16.ld if raw16 else 0, stream), "gn_apply")
        return y

    def lnorm(self, x: _V, nkey, out: _V, eps=1e-5) -> None:
        """LayerNorm of 16-bit or fp32 rows -> 16-bit rows (gamma ``nkey.g``, beta ``nkey.b``)"""
        args = (x.p, x.rows, x.C, x.ld, self.wp(nkey + ".g"), self.wp(nkey + ".b"), eps, out.p, out.ld)
        if x.es == 2:
            self.emit(self.lib.mi355x_sd_layernorm, args + (self.stream,), "ln")
        else:
            self.emit(self.lib.mi355x_sd_layernorm_ex, args + (1, self.stream), "ln")

    def sdpa(self, q: _V, k: _V, v: _V, out: _V, heads, sq, skv, bias=None, bias_strides=(0, 0, 0), scale=None,
             fn: Optional[Callable] = None, tail=(), suffix="") -> None:
        """softmax(q k^T * scale + bias) v per (batch, head); sq / skv rows per batch item. ``bias``: fp32, element strides (batch, head,
        query). ``scale``: head_dim^-0.5 unless given. ``fn`` + ``tail``: mi355x_sd_sdpa_ex / _accum and what they take before the stream."""
        B, d = self.B, q.C // heads
        self.emit(fn or self.lib.mi355x_sd_sdpa,
                  (q.p, k.p, v.p, bias, out.p, B, heads, sq, skv, d, sq * q.ld, q.ld, skv * k.ld, k.ld, skv * v.ld, v.ld, sq * out.ld,
                   out.ld, *bias_strides, d ** -0.5 if scale is None else scale, *tail, self.stream), "attn",
                  4.0 * B * heads * sq * skv * d, f"{B}x{heads}x{sq}x{skv}x{d}{suffix}")


# Test plumbing, ONE place: while a backend object is pushed here (tests/abi_emulator.py ``on_emulator`` does that around a
# constructor call), models built meanwhile send their C-ABI calls to it instead of the HIP library -- the host logic of every
# model then runs on a machine without a GPU. Product code never pushes anything: the library is the only backend it selects, and
# a missing library or GPU is an error, not a fallback.
# A context variable, not a module global: the override is seen by the thread / task that set it and by nobody else (a model built
# meanwhile on another thread gets the HIP library), and it must be an object that SAYS it is a test backend.
_BACKEND_OVERRIDE: contextvars.ContextVar = contextvars.ContextVar("mi355x_sd_test_backend", default=None)


@contextlib.contextmanager
def crossing(stream, device):
    """The body runs with ``stream`` current, ordered after what the caller's current stream on ``device`` holds so far; what the
    caller enqueues afterwards is ordered after the body. ``stream`` None (the emulated backend): nothing. The trailing wait is not
    in a ``finally``: an exception in the body propagates with nothing enqueued behind it."""
    if stream is None:
        yield
        return
    cur = torch.cuda.current_stream(device)
    stream.wait_stream(cur)
    with torch.cuda.stream(stream):
        yield
    cur.wait_stream(stream)


def caller_stream(device, emulated: bool = False) -> int:
    """the caller's current stream on ``device`` as the C ABI takes it (0 on the emulated backend)"""
    return 0 if emulated else torch.cuda.current_stream(device).cuda_stream


class DeviceProgram:
    """Backend selection + execution of a plan (``plan.prog``: list of (cfunc, args, kind, flops))."""

    def _init_backend(self, device, use_graph: bool, profile: bool):
        _test_backend = _BACKEND_OVERRIDE.get()
        if _test_backend is not None and not getattr(_test_backend, "IS_TEST_BACKEND", False):
            raise TypeError("paddlemix_amd.program._BACKEND_OVERRIDE holds something that is not a test backend")
        self._emulated = _test_backend is not None
        if self._emulated:
            self._lib = _test_backend
            self.device = torch.device("cpu")
            self._stream = None
            self._stream_ptr = 0
            self._gemm_ws = (None, 0)
            use_graph = False
        else:
            self._lib = _lib.load()  # hard failure if the HIP library is not built
            if not torch.cuda.is_available():
                raise _lib.MI355XError(f"{type(self).__name__}(mi355x) needs a GPU; there is no CPU fallback")
            self.device = torch.device(device)
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            _lib.check(self._lib.mi355x_sd_init(self.device.index))
            self._stream = torch.cuda.Stream(device=self.device)
            self._stream_ptr = self._stream.cuda_stream
            # split-K / widening scratch of this model's GEMM-class launches: owned here, an ARGUMENT of every such call the planners
            # emit (`*self._gemm_ws` in front of the stream; ABI 12 -- nothing process-wide is bound), baked into the graphs
            self._workspace = torch.empty(WORKSPACE_BYTES, device=self.device, dtype=torch.uint8)
            self._gemm_ws = (self._workspace.data_ptr(), self._workspace.numel())
        self.dtype = _lib.elem_dtype()
        self.use_graph = use_graph
        self.profile = profile
        self._plans: Dict[tuple, _Plan] = {}
        self.w: Dict[str, torch.Tensor] = {}
        self.kernel_times: Dict[str, list] = {}

    def plan_for(self, key, build: Callable[[], _Plan]) -> _Plan:
        """the cached plan of ``key``, built by ``build()`` the first time it is asked for"""
        if key not in self._plans:
            self._plans[key] = build()
        return self._plans[key]

    def weight_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.w.values())

    def _run_eager(self, plan: _Plan) -> None:
        if not self.profile or self._emulated:
            for fn, args, _, _ in plan.prog:
                rc = fn(*args)
                if rc:
                    _lib.check(rc)
            return
        evs = []
        for fn, args, kind, fl in plan.prog:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(self._stream)
            rc = fn(*args)
            e1.record(self._stream)
            if rc:
                _lib.check(rc)
            evs.append((kind, fl, e0, e1))
        self._stream.synchronize()
        for kind, fl, e0, e1 in evs:
            self.kernel_times.setdefault(kind, []).append((e0.elapsed_time(e1) * 1e-3, fl))

    def _capture(self, plan: _Plan) -> None:
        lib = self._lib
        sp = self._stream_ptr
        _lib.check(lib.mi355x_sd_graph_begin(sp))
        try:
            for fn, args, _, _ in plan.prog:
                rc = fn(*args)
                if rc:
                    _lib.check(rc)
        finally:
            exe = ctypes.c_void_p()
            rc = lib.mi355x_sd_graph_end(sp, ctypes.byref(exe))
        _lib.check(rc)
        plan.graph = exe

    def run(self, plan: _Plan) -> torch.Tensor:
        """Launch the step on the model's stream (inputs already staged); returns the static output buffer."""
        if self.use_graph and not self.profile:
            if plan.graph is None:
                self._run_eager(plan)  # warm-up outside capture (lazy module loading)
                self._capture(plan)
            _lib.check(self._lib.mi355x_sd_graph_launch(plan.graph, self._stream_ptr))
        else:
            self._run_eager(plan)
        return plan.out

    def on_stream(self):
        """``with self.on_stream():`` -- the body runs on the model's stream, between the caller's work before and after it"""
        return crossing(self._stream, self.device)

    def run_staged(self, plan: _Plan, stage) -> torch.Tensor:
        """``stage(non_blocking)`` (the copies into the plan's static inputs), then ``run(plan)``, both on the model's stream"""
        with self.on_stream():
            stage(not self._emulated)
            return self.run(plan)

    def require_gpu(self, *tensors) -> None:
        if not self._emulated and not all(t.is_cuda for t in tensors):
            raise _lib.MI355XError("inputs must be GPU tensors (no CPU fallback)")

    def caller_stream(self) -> int:
        return caller_stream(self.device, self._emulated)
