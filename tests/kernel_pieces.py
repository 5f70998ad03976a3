"""What the kernel families' case-matrix children (tests/*_child.py) share: the buffers that prove a kernel wrote exactly its
output and read only its input, and the loop that runs a case table. Child side: imports torch; buffers live on "cuda" unless a
device is given (tests/test_kernel_pieces.py runs them on the CPU).

An output is a view inside a flat buffer of canary bits -- a NaN pattern of the element type, never a result -- and
Guarded.counts() tells how many elements of the view still hold the canary (unwritten) and how many outside it no longer do
(overwritten). An input is a view inside a NaN buffer (nan_embed): a read outside it poisons the result.

The geometry -- row gaps, base offsets, rows behind the end, tails -- decides which store form and which route a case takes. It is
part of the case: every number is an argument the family passes, none is a default here."""
import torch

from tests.gpu_child import Routes, emit

CANARY16 = 0x7FA5        # a NaN bit pattern in bf16 and in fp16
CANARY32 = 0x7FA5A5A5    # ... in fp32
CANARY8 = 0xA5           # plain bytes
F8_NAN = 0x7F            # NaN in e4m3fn (finite inputs saturate to 448): the byte canary of the W8A8 family's e4m3 output
_BITS = {16: torch.int16, 32: torch.int32, 8: torch.uint8}
_CANARY = {16: CANARY16, 32: CANARY32, 8: CANARY8}


def row_strides(shape, ld):
    """strides of a [rows, C] or [B, HW, C] view whose rows lie ld elements apart"""
    return tuple(ld * (shape[1] if len(shape) == 3 and i == 0 else 1) for i in range(len(shape) - 1)) + (1,)


def counts(bits, inside, canary):
    """(unwritten, overwritten): elements of the mask `inside` that still hold the canary, elements outside it that no longer do"""
    return int(((bits == canary) & inside).sum().item()), int(((bits != canary) & ~inside).sum().item())


class Guarded:
    """an output inside a flat canary buffer of n elements of `kind` (16, 32 or 8) bits. bits: the flat integer buffer; buf: the same
    memory as dt (16 bits: the build's element type; 32: fp32; 8: the bytes); inside: bool mask of the output's elements; view: the
    output (strided, rows, block) or a gathered copy of it (at: the kernel gets `ptr`)."""
    def __init__(self, n, kind, dt=None, device="cuda", canary=None):
        self.canary = _CANARY[kind] if canary is None else canary
        self.bits = torch.full((n,), self.canary, dtype=_BITS[kind], device=device)
        self.buf = self.bits if kind == 8 else self.bits.view(torch.float32 if kind == 32 else dt)
        self.inside = torch.zeros(n, dtype=torch.bool, device=device)

    @classmethod
    def strided(cls, shape, strides, off, n, kind, **kw):
        """a view of `shape` and `strides` that starts `off` elements into the buffer"""
        g = cls(n, kind, **kw)
        g.view = g.buf.as_strided(tuple(shape), tuple(strides), off)
        g.inside.as_strided(tuple(shape), tuple(strides), off).fill_(True)
        return g

    @classmethod
    def rows(cls, shape, ld, kind, *, extra_rows, tail, **kw):
        """a [rows, C] or [B, HW, C] view with row stride ld at the start of the buffer, extra_rows rows and tail elements behind"""
        rows = 1
        for s in shape[:-1]:
            rows *= s
        return cls.strided(shape, row_strides(shape, ld), 0, (rows + extra_rows) * ld + tail, kind, **kw)

    @classmethod
    def block(cls, M, N, kind, *, above, below, left, right, **kw):
        """an [M, N] block inside an [above + M + below, left + N + right] canary block"""
        ld = left + N + right
        return cls.strided((M, N), (ld, 1), above * ld + left, (above + M + below) * ld, kind, **kw)

    @classmethod
    def at(cls, idx, n, kind, *, base, **kw):
        """the elements `idx` (an index tensor of the output's shape) of the buffer; ptr: the address of element `base`"""
        g = cls(n, kind, **kw)
        g.idx = idx
        g.inside[idx] = True
        g.ptr = g.buf.data_ptr() + base * g.buf.element_size()
        return g

    def get(self):   # (at) the output's elements, gathered
        return self.buf[self.idx]

    def counts(self):   # (unwritten, overwritten)
        return counts(self.bits, self.inside, self.canary)


def nan_embed(vals, strides, off, n):
    """vals as a view with `strides`, `off` elements into a flat NaN buffer of n elements on vals' device: (view, flat buffer).
    Covers a strided row view (nan_rows), a flat vector followed by NaN and NaN margins around a dense tensor."""
    buf = torch.full((n,), float("nan"), dtype=vals.dtype, device=vals.device)
    view = buf.as_strided(tuple(vals.shape), tuple(strides), off)
    view.copy_(vals)
    return view, buf


def nan_rows(vals, ld, *, tail):
    """vals [..., C] as a view with row stride ld (the gaps ld > C hold NaN), `tail` NaN elements behind the last row"""
    return nan_embed(vals, row_strides(tuple(vals.shape), ld), 0, vals.numel() // vals.shape[-1] * ld + tail)[0]


def run_cases(cases, run_case, *, route_log, tag, names):
    """a child's main: every case of `names` (none: of `cases`) through run_case(name) -> dict, one after another on device 0;
    with a route_log (the environment variable of a debug-build route log) each result gets the lines its launches logged as
    "route". Emits {name: result} under `tag`. Nothing is caught: an exception ends the child."""
    from paddlemix_amd import ops
    ops.init(0)
    routes = Routes(route_log) if route_log else None
    if routes:
        routes.take()
    res = {}
    for name in names or cases:
        res[name] = run_case(name)
        if routes:
            res[name]["route"] = routes.take()
        torch.cuda.empty_cache()
    emit(tag, res)
