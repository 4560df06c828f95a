"""Shared pieces of the ABI tests (a plain module, like sweep_cases.py): the prototypes of include/dojo_hip.h parsed into ctypes kinds, and the
layout (sizeof, ordered member offsets) of a struct of the header as a C compiler sees it."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dojo_hip.h")
LIBRARY = os.path.join(ROOT, "dojo.jl_amd", "csrc", "libdojo_hip.so")
JULIA_SHIM = os.path.join(ROOT, "dojo.jl_amd", "julia", "DojoHIP.jl")



def text(path):
    """the text of a file of the repository (a path relative to its root, or absolute)"""
    return open(os.path.join(ROOT, path)).read()


def host_source(module):
    """the source of dojo_amd/<module>.py (importing autograd, ilqr or envs needs torch: the text is enough for a signature check)"""
    return text(os.path.join("dojo.jl_amd", "host", "dojo_amd", module + ".py"))


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}


def _code(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _kind(decl):
    """the ctypes kind of one parameter or return type: every pointer, array and DojoHandle is a c_void_p"""
    decl = decl.strip()
    if "*" in decl or "[" in decl or decl.startswith("DojoHandle"):
        return C.c_void_p
    return _SCALARS[decl.replace("const ", "").split()[0]]


def header_prototypes():
    """-> [(restype, name, [argtype, ..])] for every `dojo_*` prototype of the header, in its order"""
    out = []
    for ret, name, params in re.findall(r"^\s*(int|void|const\s+char\s*\*)\s*(dojo_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", _code(text(HEADER)), flags=re.M):
        ret = " ".join(ret.split())
        restype = None if ret == "void" else C.c_char_p if "char" in ret else C.c_int
        params = " ".join(params.split())
        out.append((restype, name, [] if params == "void" else [_kind(p) for p in params.split(",")]))
    return out


def header_struct_members(struct_name):
    """the member names of `typedef struct <struct_name> { .. }` in declaration order"""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct_name, struct_name), _code(text(HEADER)), flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            first, *rest = decl.split(",")
            names += [re.sub(r"\[.*", "", d).replace("*", " ").split()[-1] for d in [first] + rest]
    return names


def c_layout(struct_name):
    """-> (sizeof, [(member, offsetof), ..] in declaration order) of a struct of the header: a host-only C program compiled against it prints them"""
    import tempfile
    members = header_struct_members(struct_name)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "dojo_hip.h"\nint main(void) {\n    printf("%%zu\\n", sizeof(%s));\n' % struct_name
                    + "".join('    printf("%%zu\\n", offsetof(%s, %s));\n' % (struct_name, m) for m in members) + "    return 0;\n}\n")
        subprocess.run(["cc", "-I" + os.path.dirname(HEADER), src, "-o", exe], check=True, capture_output=True, text=True, timeout=120)
        vals = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    return vals[0], list(zip(members, vals[1:]))


def mirror_layout(cls):
    """(sizeof, [(member, offset), ..]) of a ctypes mirror, to compare with c_layout"""
    return C.sizeof(cls), [(f[0], getattr(cls, f[0]).offset) for f in cls._fields_]


def assert_declared(names):
    """the header declares each as `int name(DojoHandle ...`"""
    for n in names:
        assert re.search(r"^int\s+%s\s*\(\s*DojoHandle\b" % n, text(HEADER), re.M), n


def assert_exported_and_bound(names):
    """the built library exports each, and api.lib() binds it with as many argtypes as the header gives it parameters (the kinds: test_signature_table_is_the_header)"""
    from dojo_amd import api
    protos = {name: args for _, name, args in header_prototypes()}
    built = C.CDLL(LIBRARY)
    for n in names:
        assert hasattr(built, n), n
        assert len(getattr(api.lib(), n).argtypes) == len(protos[n]), n


def assert_mirror_layout(struct_name, mirror, fields=None):
    """the ctypes mirror has the size, the member names (`fields`, when the caller states them) and the ordered offsets the C compiler gives the struct"""
    assert re.search(r"typedef\s+struct\s+%s\s*\{" % struct_name, text(HEADER))
    if fields is not None:
        assert [f[0] for f in mirror._fields_] == list(fields)
    assert mirror_layout(mirror) == c_layout(struct_name)
