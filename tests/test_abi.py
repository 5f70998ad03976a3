"""The C-ABI library loads and exports exactly the symbols include/mi355x_sd.h declares, the binding gives each of them the header's
types, and the exported-program runtime knows every launch of the header (no compute, no GPU)."""
import ctypes
import os
import re
import struct

import pytest

from paddlemix_amd import _lib
from tests.header_decls import declared, launches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_VALUE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "int32_t": ctypes.c_int32}


def _declared():
    return sorted(declared())


def _is_pointer_type(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer)


def _fits(ctype, kind):
    """the binding's type against a parameter (or return) type of the header"""
    if kind in BY_VALUE:
        return ctype is BY_VALUE[kind]
    assert kind.endswith("*"), kind
    if kind == "const char*":
        return ctype is ctypes.c_char_p
    inner = kind[:-1].strip()
    if inner.endswith("const"):
        inner = inner[:-len("const")].strip()
    if inner.endswith("*"):                                  # T**: a POINTER of a pointer type
        return issubclass(ctype, ctypes._Pointer) and _is_pointer_type(ctype._type_)
    base = inner[len("const "):] if inner.startswith("const ") else inner
    return ctype is ctypes.c_void_p or (issubclass(ctype, ctypes._Pointer) and ctype._type_ is BY_VALUE.get(base))


def test_header_and_binding_agree():
    assert _declared() == sorted(_lib.SIGNATURES)
    for name, (ret, params) in declared().items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert _fits(restype, ret), (name, ret, restype)
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for ctype, (kind, pname) in zip(argtypes, params):
            assert _fits(ctype, kind), (name, pname, kind, ctype)


def test_the_type_rule_refuses_what_would_load_and_pass_by_name():
    """what the comparison is for: an `int` bound where the header says `int64_t`, a data pointer bound as a string, one level of
    indirection too few"""
    assert not _fits(ctypes.c_int, "int64_t") and not _fits(ctypes.c_int64, "int") and not _fits(ctypes.c_int, "float")
    assert not _fits(ctypes.c_int64, "size_t") and not _fits(ctypes.c_void_p, "int") and not _fits(ctypes.c_int, "void*")
    assert not _fits(ctypes.c_void_p, "const char*") and not _fits(ctypes.c_char_p, "const void*")
    assert not _fits(ctypes.POINTER(ctypes.c_int), "int64_t*") and _fits(ctypes.POINTER(ctypes.c_int64), "const int64_t*")
    assert not _fits(ctypes.c_void_p, "void**") and not _fits(ctypes.POINTER(ctypes.c_int), "void**")
    assert _fits(ctypes.POINTER(ctypes.c_void_p), "const float* const*") and _fits(ctypes.POINTER(ctypes.c_char_p), "const char**")


def _one_launch_program(name, params):
    """a program file of one launch of `name` (the layout: paddlemix_amd/export.py): no region, no I/O; integers and floats 0, pointers
    tagged null, the stream tagged as the stream"""
    a_int, a_float, a_null, a_stream = 0, 1, 3, 4
    tags = [a_int if kind in ("int", "int64_t", "size_t") else a_float if kind == "float" else a_null for kind, _ in params]
    assert all(kind.endswith("*") for (kind, _), t in zip(params, tags) if t == a_null), name
    if params and params[-1] == ("void*", "stream"):
        tags[-1] = a_stream
    sym = name.encode()
    return (b"MI3SDPRG" + struct.pack("<IIIIIIQ", 1, _lib.ABI_VERSION, _lib._BUILDS[_lib.ELEM_NAME][1], 0, 1, 0, 0) +
            struct.pack("<I", len(sym)) + sym + struct.pack("<I", len(tags)) + b"".join(struct.pack("<IQQ", t, 0, 0) for t in tags))


def test_replay_table_knows_every_launch_of_the_header(tmp_path):
    """csrc/program_exec.hip op_table(): paddlemix_amd/export.py writes any entry a planner emits, so the C loader must know every one
    a planner could -- every function of the header whose last parameter is `void* stream`, bar the handle and runtime entries"""
    from paddlemix_amd.export import ExportedProgram
    assert {"mi355x_sd_linear", "mi355x_sd_relu", "mi355x_sd_tile_blend", "mi355x_sd_plms_update"} <= set(launches())
    path = str(tmp_path / "one.mi3prg")
    for name in launches():
        open(path, "wb").write(_one_launch_program(name, declared()[name][1]))
        prog = ExportedProgram(path)                # mi355x_sd_program_load: finds the entry and type-checks the launch against it
        assert prog.num_launches == 1, name
        prog.close()
    assert "mi355x_sd_graph_begin" not in launches()
    open(path, "wb").write(_one_launch_program("mi355x_sd_graph_begin", declared()["mi355x_sd_graph_begin"][1]))
    with pytest.raises(_lib.MI355XError, match="unknown entry point 'mi355x_sd_graph_begin'"):
        ExportedProgram(path)


def test_library_loads_and_exports_everything():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    for name in _declared():
        assert hasattr(lib, name), name
    assert lib.mi355x_sd_abi_version() == _lib.ABI_VERSION
    assert isinstance(lib.mi355x_sd_last_error(), bytes)
    # pure host-side helper: no device needed
    assert lib.mi355x_sd_groupnorm_workspace_floats(8, 16384, 320) > 0


def test_missing_library_is_loud(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libmi355x_sd.so")
    with pytest.raises(_lib.MI355XError, match="no CPU"):
        _lib.load()


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "paddlemix_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f
                assert not re.search(r"^\s*(from|import)\s+tests\b", txt, flags=re.M), f


def test_early_residual_kernels_keep_their_landing_registers():
    """csrc/gemm_pipe.hip gemm_pipe_pre_kernel: the residual rows land in v216 .. v255 through hand-written loads; nothing the
    compiler generated may name those registers (amdgpu_num_vgpr(216) is a budget, not a reservation -- round 4 hit exactly
    that). Disassembles both built libraries; no GPU needed."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tools = [os.path.join("/opt/rocm/lib/llvm/bin", t) for t in ("llvm-objdump", "llvm-objcopy")]
    libs = [os.path.join(root, "paddlemix_amd", n) for n in ("libmi355x_sd.so", "libmi355x_sd_f16.so", "libmi355x_sd_dbg.so")]
    if not all(os.path.exists(t) for t in tools + libs):
        pytest.skip("needs the ROCm LLVM tools and both built libraries")
    p = subprocess.run([sys.executable, os.path.join(root, "scripts", "check_landing_zone.py")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    import re
    # the kernels are recognised by the marker instruction their epilogue emits, not by name
    found = re.findall(r"(\d+) kernels with the landing-zone marker, (\d+) compiler-generated uses", p.stdout)
    assert len(found) == 3 and all(int(n) >= 3 and int(bad) == 0 for n, bad in found), p.stdout


def test_groupnorm_act_fits_is_the_launchers_whole_contract():
    """mi355x_sd_groupnorm_act_fits == 1 must mean mi355x_sd_groupnorm_act runs (the planners choose the one-launch form on the
    predicate alone): wide groups (C / groups > 128: the kernel's per-group gamma / beta table) are refused by the predicate itself,
    in the built library and in the C-ABI emulator alike -- a norm_num_groups = 8 model at C = 1280 then plans statistics + apply."""
    from paddlemix_amd import _lib
    from tests.abi_emulator import Emulator
    lib, emu = _lib.load(), Emulator()
    for hw, c, groups, want in ((256, 1280, 32, 1), (256, 1280, 8, 0), (64, 2048, 8, 0), (64, 2048, 16, 1), (1 << 16, 320, 32, 0),
                                (256, 1290, 30, 0)):
        assert lib.mi355x_sd_groupnorm_act_fits(hw, c, groups) == want, (hw, c, groups)
        assert emu.mi355x_sd_groupnorm_act_fits(hw, c, groups) == want, (hw, c, groups)


def test_emulator_answers_the_planners_size_queries_like_the_library():
    """A model planned on the emulator can be exported and replayed on the device (tests/test_gpu_export.py): every size the planner
    asks the backend for must be the library's own answer. (Round 4: the emulator's GroupNorm workspace was 64 floats flat, the
    device kernel writes up to thousands -- a CPU-planned VAE program then failed one run in three on the device.)"""
    from paddlemix_amd import _lib
    from tests.abi_emulator import Emulator
    lib, emu = _lib.load(), Emulator()
    for B, HW, C in ((2, 1024, 32), (2, 256, 64), (2, 64, 64), (8, 16384, 128), (1, 4096, 320), (8, 1024, 1280), (3, 100, 2560), (1, 7, 8)):
        assert emu.mi355x_sd_groupnorm_workspace_floats(B, HW, C) == lib.mi355x_sd_groupnorm_workspace_floats(B, HW, C), (B, HW, C)


@pytest.mark.parametrize("src", ["tests/c/unet_exec_test.c", "tests/c/program_test.c", "scripts/c/step_bench.c", "scripts/c/gemm_probe.c",
                                 "scripts/c/conv_probe.c", "scripts/c/attn_probe.c", "tests/c/comm_test.c"])
def test_plain_c_clients_build_against_the_header_and_fail_loudly_without_a_device(src, tmp_path):
    """Every plain-C client of the ABI (the two GPU-test clients and the torch-free benches / probes) compiles against include/mi355x_sd.h
    as C11, links against the library, and -- on a machine without a GPU -- exits non-zero with the library's own message instead
    of computing anything anywhere else."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("no gcc / ROCm headers")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    exe = str(tmp_path / "client")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "scripts", "c"), os.path.join(ROOT, src), "-L" + libdir, "-lmi355x_sd", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    import torch
    if torch.cuda.is_available():
        return
    cfg = os.path.join(ROOT, "scripts", "c", "sd15_unet_config.json")
    args = {"tests/c/unet_exec_test.c": [cfg, "1", "8", "8", "7", str(tmp_path / "o.bin")], "tests/c/program_test.c": [str(tmp_path / "none.prog")],
            "scripts/c/step_bench.c": [cfg, "1", "8", "8", "7", "1", "0"], "scripts/c/gemm_probe.c": ["1"], "scripts/c/conv_probe.c": ["1"],
            "scripts/c/attn_probe.c": ["1"], "tests/c/comm_test.c": ["0", "1", str(tmp_path / "id.bin")]}[src]
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH=libdir), timeout=120)
    assert r.returncode != 0, r.stdout
    assert r.stderr.strip(), "a failing client says why"


def test_c_bench_configs_are_the_bench_workloads():
    """scripts/c/*_unet_config.json (what scripts/c/step_bench.c plans) are the configurations bench.py's workloads name."""
    import json
    from tests.configs import SD15, SDXL
    for name, cfg in (("sdxl", SDXL), ("sd15", SD15)):
        got = json.load(open(os.path.join(ROOT, "scripts", "c", f"{name}_unet_config.json")))
        assert got == {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, name
