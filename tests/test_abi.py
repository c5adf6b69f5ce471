"""CPU: the C-ABI library loads here (no GPU, no compute calls) and exports every symbol that
include/mi355x_rec.h declares, with the argument counts the ctypes binding assumes."""
import ctypes
import inspect
import os
import re
import subprocess

from mi355x_rec import _lib
from tests.cpu_kernels import NumpyKernels
from tests.util import _header_decls


def test_header_binding_and_library_agree(lib):
    decls = _header_decls()
    assert len(decls) >= 30
    assert set(decls) == set(_lib.SIGNATURES), set(decls) ^ set(_lib.SIGNATURES)
    for name, nargs in decls.items():
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (mi_\w+)", out))
    assert set(decls) <= exported
    # nothing but the C ABI leaks out of the library
    assert all(s.startswith("mi_") for s in exported), exported


def test_numpy_stand_ins_take_what_the_binding_passes():
    """tests/cpu_kernels.py: the engine calls a stand-in with the arguments it gives the binding, positionally — every
    SIGNATURES argument but the stream, which the binding adds"""
    stand_ins = {n: f for n, f in vars(NumpyKernels).items() if n.startswith("mi_")}
    assert len(stand_ins) >= 41
    for name, f in stand_ins.items():
        assert name in _lib.SIGNATURES, name
        params = list(inspect.signature(f).parameters.values())[1:]               # (self)
        assert all(p.kind == p.POSITIONAL_OR_KEYWORD for p in params), (name, [str(p) for p in params])
        assert len(params) == len(_lib.SIGNATURES[name][1]) - 1, (name, len(params), len(_lib.SIGNATURES[name][1]) - 1)


def test_the_fused_model_struct_is_laid_out_as_the_c_compiler_lays_it_out(tmp_path):
    """host only: the header through the system's C compiler; the ctypes mirror must agree on the size and on the offset of the
    last field (every field before it then has room for nothing else than its own type)"""
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mi355x_rec.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(mi_fused_model_t), offsetof(mi_fused_model_t, wide_fields)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", header, str(src), "-o", str(exe)], check=True)
    size, off = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert (size, off) == (ctypes.sizeof(_lib.FusedModel), _lib.FusedModel.wide_fields.offset)
    assert [n for n, _ in _lib.FusedModel._fields_][-1] == "wide_fields"


def test_library_identity(lib):
    assert lib.mi_abi_version() == _lib.ABI_VERSION
    assert b"gfx950" in lib.mi_build_info()
    assert lib.mi_last_error() is not None


def test_only_gfx950_code_objects():
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "--list", "--type=o",
                          "--input=" + _lib.LIB_PATH], capture_output=True, text=True)
    if out.returncode == 0 and out.stdout.strip():
        targets = [t for t in out.stdout.split() if "amdgcn" in t]
        assert targets and all("gfx950" in t for t in targets), targets


def test_shipped_library_reads_no_environment_variables():
    """tuning switches live in the tools' build (make -C csrc tuning, -DMI_TUNING) only — the product
    library does not even import getenv."""
    out = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "getenv" not in out
