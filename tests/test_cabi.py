"""C-ABI surface checks (CPU-safe: loads the library, no compute calls)."""
import ctypes
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "ballista_gpu.h")


INTERNAL_HEADER = os.path.join(ROOT, "datafusion_ballista_amd", "csrc",
                               "bg_internal.h")


def _strip_comments(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def header_prototypes(path=HEADER):
    """{name: (return type, [parameter types])} of every function a header
    declares, types as written with whitespace squeezed out."""
    protos = {}
    for ret, name, params in re.findall(
            r"^\s*((?:const\s+)?\w+[\s*]+)(bg_\w+)\s*\(([^)]*)\)\s*;",
            _strip_comments(path), flags=re.M):
        types = []
        if params.strip() != "void":
            for prm in params.split(","):
                # drop the parameter's name: the last identifier
                types.append(re.sub(r"\w+\s*$", "", prm.strip()))
        protos[name] = tuple(re.sub(r"\s+", "", t) for t in [ret] + types)
    return protos


def header_symbols():
    """Every function declared in include/ballista_gpu.h."""
    syms = list(header_prototypes())
    assert len(syms) >= 15
    return syms


def header_structs():
    """{typedef name: [field names in order]} of every struct in the header."""
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;",
                                 _strip_comments(HEADER), flags=re.S):
        structs[name] = [re.search(r"(\w+)\s*$", decl).group(1)
                         for decl in body.split(";") if decl.strip()]
    return structs


def _gpu_struct_classes(gpu):
    return {n: c for n, c in vars(gpu).items()
            if isinstance(c, type) and issubclass(c, ctypes.Structure)
            and c is not ctypes.Structure}


def test_struct_layouts_match_header(tmp_path):
    """Every typedef struct of the header has a gpu.Bg* ctypes class (and
    vice versa) with the same size, field names in order and offsets — as
    the host C compiler lays the header out."""
    import shutil
    import subprocess
    from datafusion_ballista_amd import gpu
    structs = header_structs()
    classes = _gpu_struct_classes(gpu)
    want_names = {"".join(w.capitalize() for w in n.split("_")): n
                  for n in structs}  # bg_page_extract_job -> BgPageExtractJob
    assert set(want_names) == set(classes)
    assert len(structs) >= 13

    prog = ["#include <stddef.h>", "#include <stdio.h>",
            '#include "ballista_gpu.h"', "int main(void) {"]
    for n, fields in structs.items():
        prog.append(f'  printf("{n} %zu\\n", sizeof({n}));')
        for f in fields:
            prog.append(f'  printf("{n}.{f} %zu\\n", offsetof({n}, {f}));')
    prog += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog) + "\n")
    cc = next((c for c in ("cc", "gcc", "clang",
                           "/opt/rocm/lib/llvm/bin/clang")
               if shutil.which(c)), None)
    assert cc, "no host C compiler found (build() needs one too)"
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-x", "c", "-I", os.path.dirname(HEADER),
                    str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run(
        [str(exe)], check=True, capture_output=True,
        text=True).stdout.splitlines())

    for cls_name, n in want_names.items():
        cls = classes[cls_name]
        assert [f[0] for f in cls._fields_] == structs[n], n
        assert ctypes.sizeof(cls) == int(got[n]), n
        for f in structs[n]:
            assert getattr(cls, f).offset == int(got[f"{n}.{f}"]), (n, f)


def _c_kind(ctype):
    """C type as written (no whitespace) -> parameter kind."""
    if ctype in ("constchar*", "char*"):
        return "char*"
    if ctype.endswith("*"):
        return "pointer"
    return {"void": "void", "int": "int32", "int32_t": "int32",
            "uint32_t": "uint32", "int64_t": "int64", "uint64_t": "uint64",
            "double": "double"}[ctype]


def _ctypes_kind(t):
    if t is None:
        return "void"
    if t is ctypes.c_char_p:
        return "char*"
    if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer):
        return "pointer"
    return {ctypes.c_int32: "int32", ctypes.c_uint32: "uint32",
            ctypes.c_int64: "int64", ctypes.c_uint64: "uint64",
            ctypes.c_double: "double"}[t]


def test_signature_table_matches_headers():
    """gpu.py's signature table declares every function of the public and
    the internal header — nothing more — with the header's arity, return
    kind and per-parameter kind; load_library() applied it."""
    from datafusion_ballista_amd import gpu
    protos = {**header_prototypes(), **header_prototypes(INTERNAL_HEADER)}
    assert len(protos) >= 80
    assert set(gpu._SIGNATURES) == set(protos)
    L = gpu.load_library()
    for name, (ret, *params) in protos.items():
        fn = getattr(L, name)
        assert _ctypes_kind(fn.restype) == _c_kind(ret), name
        assert [_ctypes_kind(t) for t in fn.argtypes] == \
            [_c_kind(t) for t in params], name


def test_64bit_arguments_need_no_wraps():
    """Declared argtypes carry a bare Python int into an int64_t parameter
    whole (undeclared, ctypes would pass a C int), and reject a call with
    a missing or mistyped argument before it reaches the library."""
    import torch
    from datafusion_ballista_amd import gpu
    L = gpu.load_library()
    # ctypes reports a missing argument as a plain TypeError and a mistyped
    # one as ctypes.ArgumentError
    with pytest.raises(TypeError, match="5 arguments"):
        L.bg_gather(None, 1 << 40, None, 1 << 40)
    with pytest.raises(ctypes.ArgumentError):
        L.bg_gather(None, 1.5, None, 1 << 40, None)
    if not torch.cuda.is_available():
        # refused at the no-GPU check, after the arguments converted; with
        # a GPU this call must not be made (it would gather 2^40 rows)
        assert L.bg_gather(None, 1 << 40, None, 1 << 40, None) == -2


def test_library_exports_every_header_symbol():
    from datafusion_ballista_amd import gpu
    L = gpu.load_library()
    for sym in header_symbols():
        assert hasattr(L, sym), f"libballista_gpu.so missing symbol {sym}"


def test_version():
    from datafusion_ballista_amd import gpu
    L = gpu.load_library()
    assert L.bg_version() >= 10


def test_committed_library_matches_committed_sources():
    """Build provenance: the library reports the sha256
    of the sources it was compiled from; recomputing it over the committed
    sources must match, so a stale committed .so fails here."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "graft_entry", os.path.join(ROOT, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from datafusion_ballista_amd import gpu
    L = gpu.load_library()
    got = L.bg_source_hash().decode()
    assert got == mod.source_hash(), (
        "libballista_gpu.so was not built from the committed sources "
        f"(lib reports {got!r}); run __graft_entry__.build()")


def test_init_fails_loudly_without_gpu():
    """On a GPU-less host bg_init must refuse (no silent CPU fallback)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present; covered by gpu-marked tests")
    from datafusion_ballista_amd import gpu
    L = gpu.load_library()
    rc = L.bg_init(0)
    assert rc == -2  # BG_ERR_NO_GPU
    msg = L.bg_last_error().decode()
    assert "no HIP device" in msg or "no gfx950" in msg


def test_compute_requires_init():
    """Compute entry points refuse before bg_init (fail-loud contract)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from datafusion_ballista_amd import gpu
    L = gpu.load_library()
    out = ctypes.c_int64()
    rc = L.bg_mask_to_indices(None, ctypes.c_int64(0), None, ctypes.byref(out))
    assert rc == -2
    assert b"fallback" in L.bg_last_error()
