"""The declarations of include/mi355x_sd.h, parsed once for the tests that hold the binding, the step-form table and the replay table
to the header -- TEST INFRASTRUCTURE ONLY: the product has no header parser.

    declared() -> {name: (return type, [(type, name), ...])}      in the header's order; types as written, whitespace collapsed
    launches() -> the names the exported-program runtime must know (csrc/program_exec.hip op_table)"""
import functools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# handles and runtime entries take a stream too, but a program never replays them; the layout probe is a test hook
NOT_REPLAYED = ("mi355x_sd_program_", "mi355x_sd_unet_", "mi355x_sd_graph_", "mi355x_sd_comm_", "mi355x_sd_probe_layouts")


@functools.lru_cache(maxsize=None)
def declared():
    src = open(os.path.join(ROOT, "include", "mi355x_sd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(mi355x_sd_\w+)\s*\(([^)]*)\)\s*;", src):
        params = [] if params.strip() == "void" else [tuple(" ".join(p.split()).rsplit(" ", 1)) for p in params.split(",")]
        assert name not in out and all(len(p) == 2 for p in params), name
        out[name] = (" ".join(ret.split()), params)
    return out


def launches():
    """every function whose last parameter is `void* stream`, except the handle / runtime entries and the layout probe"""
    return [name for name, (_, params) in declared().items()
            if params and params[-1] == ("void*", "stream") and not name.startswith(NOT_REPLAYED)]
