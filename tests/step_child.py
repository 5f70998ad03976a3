"""What the GPU children of the eight fused-step families share
(tests/{guidance,multistep,unipc,ancestral,heun,dpm2,plms,singlestep}_child.py), beside tests/gpu_child.py: canary-backed views, the shape of a
captured graph, one captured launch, the refusal runner and main(). Each child keeps its cases' launches, its state, its refusal table, its graph rows and its JSON keys."""
import ctypes
import sys
import time

import torch

from paddlemix_amd import _lib, ops
from tests.gpu_child import emit
from tests.kernel_pieces import CANARY32
from tests.kernel_pieces import counts as _counts
from tests.step_forms import TAIL

PAD = 64   # elements (256 bytes) of canary / NaN in front of and behind every view


def _in(vals, off=0):
    """the values inside a NaN buffer, `off` elements past a 16-byte boundary"""
    n = vals.numel()
    buf = torch.full((n + 2 * PAD,), float("nan"), device="cuda")
    buf[PAD + off:PAD + off + n] = vals.reshape(-1).cuda()
    return buf[PAD + off:PAD + off + n]


def _out(n, off=0):
    """(view of n floats inside a canary buffer, its bits, the mask of the view)"""
    bits = torch.full((n + 2 * PAD,), CANARY32, dtype=torch.int32, device="cuda")
    inside = torch.zeros(n + 2 * PAD, dtype=torch.bool, device="cuda")
    inside[PAD + off:PAD + off + n] = True
    return bits.view(torch.float32)[PAD + off:PAD + off + n], bits, inside


def tally(res, bits, inside):
    """adds a canary buffer's unwritten elements of the view and overwritten elements around it to res"""
    uw, ow = _counts(bits, inside, CANARY32)
    res["unwritten"] += uw
    res["overwritten"] += ow


def overwritten(bits, inside):
    """the elements around a canary buffer's view that no longer hold the canary"""
    return _counts(bits, inside, CANARY32)[1]


def launched(name, rc):
    """a launch's status; MI355X_SD_ERR_HIP ends the child: nothing more is launched after a device error"""
    if rc == 3:
        raise RuntimeError(f"{name}: MI355X_SD_ERR_HIP at launch")
    torch.cuda.synchronize()
    return rc


def _graph_shape(g):
    """(nodes, root nodes, edges) of a captured graph, asked of the HIP runtime the process already has loaded"""
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    hip = ctypes.CDLL(path)
    graph = ctypes.c_void_p(g.raw_cuda_graph())
    got = []
    for fn, args in ((hip.hipGraphGetNodes, (None,)), (hip.hipGraphGetRootNodes, (None,)), (hip.hipGraphGetEdges, (None, None))):
        k = ctypes.c_size_t(0)
        fn.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * len(args) + [ctypes.POINTER(ctypes.c_size_t)]
        fn.restype = ctypes.c_int
        assert fn(graph, *args, ctypes.byref(k)) == 0, fn
        got.append(k.value)
    return got


def capture(res, launch):
    """captures ``launch(stream)`` (one entry call -> its status) on a side stream: res gets rc and the graph's nodes / roots / edges
    -> the instantiated graph, nothing replayed yet"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, stream=s):
        res["rc"] = launch(torch.cuda.current_stream().cuda_stream)
    res["nodes"], res["roots"], res["edges"] = _graph_shape(g)
    g.instantiate()
    return g


def replay_rows(g, cur, table, state, direct, before_row=None):
    """replays the captured launch once per row of `table`, the row copied into `cur` (and before_row(i) run) first -> the elements
    of `state` (the buffers the launch updates) that differ from what the direct launches left, direct[i], summed over the rows"""
    from tests.rowmap_bounds import exact_off
    off = 0
    for i in range(len(table)):
        cur.copy_(table[i])
        if before_row:
            before_row(i)
        g.replay()
        torch.cuda.synchronize()
        off += sum(exact_off(a, b) for a, b in zip(state, direct[i]))
    return off


def refusals(form, planes, slots, deviations):
    """Every deviation from one valid call must be refused and launch nothing. The operands of `form` sit at plane slots[k] of one
    buffer of `planes` x 4096 floats filled with 7.25; the valid call is batch 1, per_sample 4096, gs 7.5, gr 0.7 (order 3).
    deviations(but, n, **addresses) -> {what: arguments}, but(**kw) being the valid call with those arguments replaced
    -> {what: status, "touched": elements of the buffer that changed}"""
    fn, st = getattr(_lib.load(), "mi355x_sd_" + form.entry), ops._stream()
    n = 4096
    buf = torch.full((planes * n,), 7.25, device="cuda")
    names = form.operands + TAIL
    addr = {k: buf.data_ptr() + 4 * n * s for k, s in zip((k for k in form.operands if k != "order"), slots)}
    ok = dict(addr, order=3, gs=7.5, gr=0.7, batch=1, n=n)

    def but(**kw):
        return tuple(kw.get(k, ok[k]) for k in names)
    res = {what: fn(*args, st) for what, args in deviations(but, n, **addr).items()}
    torch.cuda.synchronize()
    res["touched"] = int((buf != 7.25).sum().item())
    return res


def main(tag, sections, pipelines):
    """runs the child: `sections` then `pipelines` ([(name, function)]; the pipelines alone with ``pipeline`` as the only
    argument), each result under its name, and prints the one JSON line. A mistake of a section's own host code is that section's
    failure; a device error ends the child."""
    t0 = time.time()
    ops.init(0)
    res = {}
    for name, fn in (pipelines if sys.argv[1:] == ["pipeline"] else list(sections) + list(pipelines)):
        try:
            res[name] = fn()
        except (ValueError, TypeError, IndexError, KeyError, AttributeError, OSError, StopIteration, ZeroDivisionError, AssertionError,
                _lib.MI355XError) as ex:
            res[name] = {"error": f"{type(ex).__name__}: {ex}"}
        torch.cuda.empty_cache()
    res["seconds"] = round(time.time() - t0, 1)
    emit(tag, res)
