"""CPU: the ctypes binding (soccernerfs_amd/_lib.py) against include/snerf.h.  The header is parsed here, independently of the binding: every
prototype's parameter and return kinds equal the signature table's and the loaded functions carry them; every struct mirror has the header's field
names, sizes and offsets (a host C program prints them); no status-returning entry is called around `call` / `_call`; a stale library fails at load."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "snerf.h")
PKG = os.path.join(ROOT, "soccernerfs_amd")
VALUE_INT = ("snerf_abi_version", "snerf_abi_revision")  # with every *_supported: the entries whose `int` is a value, not a status


def _code():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"^\s*#.*$", "", txt, flags=re.M)


def _param_kind(p):
    p = p.strip()
    if "*" in p or p.startswith("snerf_stream_t"):
        return "P"
    return {"int32_t": "I", "int": "I", "int64_t": "L", "float": "F"}[p.split()[0]]  # a KeyError is a parameter type this file does not know


def header_signatures():
    """{name: "r:kinds"} for every prototype of the header, in the spelling of _lib.SIGNATURES."""
    code = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", "", _code(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"(const\s+char\s*\*|int64_t|int)\s+(snerf_\w+)\s*\(([^)]*)\)\s*;", code):
        if ret == "int":
            r = "i" if name in VALUE_INT or name.endswith("_supported") else "s"
        else:
            r = "l" if ret == "int64_t" else "z"
        kinds = "" if params.strip() == "void" else "".join(_param_kind(p) for p in params.split(","))
        assert name not in out, name
        out[name] = r + ":" + kinds
    assert len(out) == len(re.findall(r"\bsnerf_\w+\s*\(", code)), "a prototype of the header is not in the regular form this parser reads"
    return out


def header_structs():
    """{struct name: [field names in order]} from the header's struct bodies."""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", _code(), flags=re.S):
        fields = []
        for decl in body.split(";"):
            if decl.strip():
                fields += [re.sub(r"\[[^\]]*\]", "", d).replace("*", " ").split()[-1] for d in decl.split(",")]
        out[name] = fields
    return out


def mirrors():
    from soccernerfs_amd import _lib

    return [c for c in vars(_lib).values() if isinstance(c, type) and issubclass(c, C.Structure) and c is not C.Structure]


def _cc():
    from soccernerfs_amd import build

    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC)))  # the tree hipcc lives in: its clang compiles host C too
    clangs = [p for p in (os.path.join(rocm, "lib", "llvm", "bin", "clang"), os.path.join(rocm, "llvm", "bin", "clang")) if os.path.exists(p)]
    cc = shutil.which("cc") or (clangs[0] if clangs else None)
    assert cc, "no host C compiler: neither cc nor the ROCm tree's clang"
    return cc


def test_table_equals_header():
    from soccernerfs_amd import _lib

    sigs = header_signatures()
    assert len(sigs) >= 121  # the parser found the prototypes (the count when this test was written); a new entry needs no edit here
    assert set(sigs) == set(_lib.SIGNATURES), (sorted(set(sigs) - set(_lib.SIGNATURES)), sorted(set(_lib.SIGNATURES) - set(sigs)))
    assert {n: s for n, s in _lib.SIGNATURES.items() if sigs[n] != s} == {}
    assert sorted(_lib.EXPORTS) == sorted(sigs)


def test_loaded_functions_carry_the_header_types():
    from soccernerfs_amd import _lib

    arg = {"P": C.c_void_p, "I": C.c_int32, "L": C.c_int64, "F": C.c_float}
    ret = {"s": C.c_int, "i": C.c_int, "l": C.c_int64, "z": C.c_char_p}
    l = _lib.lib()
    for name, sig in header_signatures().items():
        fn = getattr(l, name)
        assert fn.restype is ret[sig[0]], name
        assert list(fn.argtypes) == [arg[k] for k in sig[2:]], name
        assert fn.errcheck is None, name  # raw entries return their code: tests assert rc < 0 with snerf_last_error()'s text


def test_raw_entries_keep_returning_their_code():
    """No errcheck hook: an argument error comes back as a negative code with its text in snerf_last_error()."""
    from soccernerfs_amd import _lib

    l = _lib.lib()
    assert l.snerf_mask_pack(None, 4096, 0, 4096, None, None, None) < 0 and b"null" in l.snerf_last_error()
    with pytest.raises(RuntimeError, match=r"libsnerf mask_pack failed \(code -\d+\)"):
        _lib.call("mask_pack", None, 4096, 0, 4096, None, None, None)


def test_int64_parameters_are_not_truncated(tmp_path):
    """A bare Python int above 2^31 reaches an int64_t parameter whole (with no argtypes it went through a C int)."""
    from soccernerfs_amd import _lib

    src = tmp_path / "echo.c"
    src.write_text("#include <stdint.h>\nint64_t echo(void* p, int64_t n, float x) { (void)p; return n + (int64_t)x; }\n")
    so = tmp_path / "libecho.so"
    subprocess.run([_cc(), "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    fn = C.CDLL(str(so)).echo
    _lib._declare(fn, "l:PLF")
    assert fn(None, 2 ** 31 + 5, 2) == 2 ** 31 + 7
    assert fn(None, -(2 ** 40), 0.0) == -(2 ** 40)


def test_struct_mirrors_name_the_header_fields():
    structs = header_structs()
    ms = mirrors()
    assert len(structs) >= 19
    assert sorted(m._c_struct_ for m in ms) == sorted(structs), "every header struct has exactly one mirror"
    for m in ms:
        assert [f[0] for f in m._fields_] == structs[m._c_struct_], m.__name__


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof and every offsetof as a host C compiler lays the header's structs out, against ctypes' layout of the mirrors."""
    ms = mirrors()
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "snerf.h"', "int main(void) {"]
    for m in ms:
        lines.append(f'  printf("{m._c_struct_} %zu\\n", sizeof({m._c_struct_}));')
        lines += [f'  printf("{m._c_struct_}.{f[0]} %zu\\n", offsetof({m._c_struct_}, {f[0]}));' for f in m._fields_]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run([_cc(), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    want = {}
    for m in ms:
        want[m._c_struct_] = str(C.sizeof(m))
        want.update({f"{m._c_struct_}.{f[0]}": str(getattr(m, f[0]).offset) for f in m._fields_})
    assert len(want) == len(ms) + sum(len(m._fields_) for m in ms)
    assert got == want, {k: (got.get(k), v) for k, v in want.items() if got.get(k) != v}


def test_status_entries_go_through_call():
    """Outside _lib.py every `.snerf_NAME(` left in the package names a value-returning entry; the status-returning ones are launched by
    _lib.call / FusedStep._call, which check the code under the entry's own name."""
    from soccernerfs_amd import _lib

    seen = 0
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        if os.path.basename(path) == "_lib.py":
            continue
        src = open(path).read()
        for name in re.findall(r"\.(snerf_\w+)\s*\(", src):
            assert _lib.SIGNATURES[name][0] != "s", (os.path.basename(path), name)
        assert not re.search(r"\.snerf_\w+\s+if\b|\.snerf_\w+\s*\)\s*\(|=\s*\w+(\.\w+)*\.snerf_\w+\s*$", src, flags=re.M), os.path.basename(path)  # a function taken first and called later
        for name in re.findall(r"""\b_?call\(\s*["'](\w+)["']""", src):
            assert _lib.SIGNATURES["snerf_" + name][0] == "s", (os.path.basename(path), name)
            seen += 1
    assert seen >= 100  # the launches are there: the scan did not pass by finding nothing


def test_stale_library_fails_at_load(tmp_path):
    from soccernerfs_amd import _lib

    src = tmp_path / "stub.c"
    src.write_text(f"int snerf_abi_version(void) {{ return {_lib.ABI_VERSION}; }}\nint snerf_abi_revision(void) {{ return {_lib.ABI_REVISION}; }}\n")
    so = tmp_path / "libstub.so"
    subprocess.run([_cc(), "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    with pytest.raises(RuntimeError, match="rebuild the library") as e:
        _lib.bind(str(so))
    msg = str(e.value)
    assert "lacks" in msg and "snerf_last_error" in msg and f"{len(_lib.SIGNATURES) - 2} in all" in msg
    assert "snerf_abi_version" not in msg.split("lacks")[1].split("(")[0]
    assert _lib.lib() is _lib.lib() and hasattr(_lib.lib(), "snerf_mask_pack")  # the product library is untouched by the failed bind
