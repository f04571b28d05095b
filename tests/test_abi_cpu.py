"""CPU-side checks of the C-ABI boundary: the built library loads and exports every symbol include/csmae.h declares
(no kernel is launched here), the Python binding table and constants match the header, csrc/ takes its constants from the header, the header is
valid C, and the product refuses to run without a GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    text = open(os.path.join(ROOT, "include", "csmae.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"(?:const char\*|int)\s+(csmae_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        args = [a.strip() for a in m.group(2).replace("\n", " ").split(",")]
        out[m.group(1)] = [] if args == ["void"] else args
    return out


def test_library_exports_every_declared_symbol():
    import csmae_hip
    assert os.path.exists(csmae_hip.LIB_PATH), "run `make` / __graft_entry__.build() first"
    lib = ctypes.CDLL(csmae_hip.LIB_PATH)
    decl = header_functions()
    assert len(decl) >= 30
    for name in decl:
        assert hasattr(lib, name), f"{name} declared in include/csmae.h but not exported"
    assert set(decl) == set(csmae_hip.exported_symbols())
    # ... and nothing else: the dynamic symbol table of the library (`nm -D`) holds exactly the declared csmae_* functions
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", csmae_hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()[-2:-1] == ["T"] and ln.split()[-1].startswith("csmae_")}
    assert exported == set(decl), (sorted(exported - set(decl)), sorted(set(decl) - exported))
    lib.csmae_abi_version.restype = ctypes.c_int
    assert lib.csmae_abi_version() == csmae_hip.ABI_VERSION == 7


def test_binding_arity_matches_header():
    import csmae_hip
    decl = header_functions()
    for name, sig in csmae_hip._SIGNATURES.items():
        assert len(sig) == len(decl[name]), (name, len(sig), decl[name])
        for ct, arg in zip(sig, decl[name]):
            if "*" in arg:
                assert ct is ctypes.c_void_p, (name, arg)
            elif arg.startswith("long long"):
                assert ct is ctypes.c_longlong, (name, arg)
            elif arg.startswith("float"):
                assert ct is ctypes.c_float, (name, arg)
            else:
                assert ct is ctypes.c_int, (name, arg)


def test_ops_refuse_cpu_tensors():
    from csmae_hip import ops
    a = torch.zeros(8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gemm(a, a, torch.zeros(8, 8))


def header_constants():
    """name -> value of every `#define CSMAE_<NAME> <int>` and every enumerator of the header's three enums"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "csmae.h")).read(), flags=re.S)
    out = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(CSMAE_\w+)\s+(-?\d+)\s*$", text, flags=re.M)}
    enums = re.findall(r"enum\s+(csmae_\w+)\s*\{(.*?)\}", text, flags=re.S)
    assert sorted(n for n, _ in enums) == ["csmae_epilogue", "csmae_loss", "csmae_status"]
    for _, body in enums:
        for item in body.split(","):
            name, _, value = item.partition("=")
            out[name.strip()] = int(value)
    return out


def test_python_constants_equal_the_headers():
    import csmae_hip
    hdr = header_constants()
    groups = {"CSMAE_EPI_": "EPI_", "CSMAE_GEMM_ROUTE_": "ROUTE_", "CSMAE_ATTN_ROUTE_": "ATTN_ROUTE_"}
    names = {"CSMAE_F32": "F32", "CSMAE_BF16": "BF16"}
    for h in hdr:
        for prefix, py in groups.items():
            if h.startswith(prefix):
                names[h] = py + h[len(prefix):]
    assert sum(h.startswith("CSMAE_EPI_") for h in names) == 8 and "CSMAE_EPI_GELU_Q8" in names and "CSMAE_EPI_DGELU_Q8" in names
    assert {"CSMAE_GEMM_ROUTE_F32", "CSMAE_GEMM_ROUTE_KSLAB", "CSMAE_ATTN_ROUTE_RESIDENT", "CSMAE_ATTN_ROUTE_STREAM", "CSMAE_ATTN_ROUTE_ANY",
            "CSMAE_ATTN_ROUTE_F32"} <= set(names)
    for h, py in names.items():
        assert getattr(csmae_hip, py) == hdr[h], (h, py)
    # ... and no EPI_ / ROUTE_ name of the package without a header constant behind it
    for py in dir(csmae_hip):
        if py.startswith(("EPI_", "ROUTE_", "ATTN_ROUTE_")):
            assert py in names.values(), py
    losses = {h[len("CSMAE_LOSS_"):].lower(): v for h, v in hdr.items() if h.startswith("CSMAE_LOSS_")}
    assert sorted(losses) == ["bce", "l1", "l2", "mae", "mse"]
    for kind, v in losses.items():
        assert csmae_hip.LOSS_KINDS[kind] == v, kind


def test_csrc_restates_no_header_constant():
    hdr = header_constants()
    csrc = os.path.join(ROOT, "cross-scale-mae_amd", "csrc")
    files = sorted(f for f in os.listdir(csrc) if f.endswith((".h", ".hip")))
    assert len(files) >= 20
    for f in files:
        text = open(os.path.join(csrc, f)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)", text, flags=re.M):
            assert m.group(1) not in hdr, f"{f} defines {m.group(1)}: include/csmae.h is the one place for it"
        if f == "common.h":
            assert re.search(r'^[ \t]*#[ \t]*include[ \t]+"[./\w]*csmae\.h"', text, flags=re.M), "csrc/common.h must include include/csmae.h"


def test_header_compiles_as_c():
    import shutil
    import subprocess
    cc = shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler (`cc`) on the path")
    r = subprocess.run([cc, "-std=c99", "-Wcomment", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "csmae.h")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
