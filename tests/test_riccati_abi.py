"""The Riccati backward pass at the ABI (CPU tier): the two entry points are declared in include/dojo_hip.h, listed in api.EXPORTED_SYMBOLS and bound with argument
types, exported by the built library, the Julia shim names the host-pointer one, and the ctypes mirror of `DojoRiccati` has the layout the C compiler gives the struct."""
import ctypes
import os
import re
import subprocess

from dojo_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dojo_riccati_dev", "dojo_riccati")
FIELDS = ("A", "Bm", "status", "lx", "lu", "lxx", "luu", "lux", "mu", "K", "kff", "fail", "dV", "Vx", "Vxx", "act_off", "na")


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dojo_hip.h")).read()
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(\s*DojoHandle\b" % n, hdr, re.M), n
    assert re.search(r"typedef\s+struct\s+DojoRiccati\s*\{", hdr)
    # the documented contract: what it mirrors, the recursion's failure rules, the determinism statement, what is not part of it
    for text in ("IterativeLQR", "examples/trajectory_optimization", "fail <- k + 1", "A_k, B_k are NOT read", "bit-identical from run to run", "Not part of it"):
        assert text in hdr, text


def test_python_binding_lists_them():
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS, n
    assert hasattr(api.BatchedMechanism, "riccati")
    src = open(os.path.join(ROOT, "dojo.jl_amd", "host", "dojo_amd", "api.py")).read()
    for n in NAMES:
        assert "L.%s.argtypes" % n in src, n
    ilqr = open(os.path.join(ROOT, "dojo.jl_amd", "host", "dojo_amd", "ilqr.py")).read()      # (importing it needs torch: the text is enough here)
    for name in ("def linearize_rollout(gm, x0, U)", "def riccati(gm, A, Bm, lx, lu, lxx, luu, lux=None, mu=None, status=None, act_off=0, na=None, value=False)",
                 "class QuadraticCost", "def solve(gm, x0, U0, cost, iters, act_off=0, na=None"):
        assert name in ilqr, name


def test_library_exports_them():
    lib = ctypes.CDLL(os.path.join(ROOT, "dojo.jl_amd", "csrc", "libdojo_hip.so"))
    for n in NAMES:
        assert hasattr(lib, n), n
    L = api.lib()
    assert len(L.dojo_riccati_dev.argtypes) == 4 and len(L.dojo_riccati.argtypes) == 3


def test_julia_shim_names_the_host_entry():
    jl = open(os.path.join(ROOT, "dojo.jl_amd", "julia", "DojoHIP.jl")).read()
    assert "fn(:dojo_riccati)" in jl and "function riccati(" in jl and "struct DojoRiccati" in jl


def test_ctypes_mirror_has_the_layout_of_the_c_struct(tmp_path):
    """a host-only C program compiled against include/dojo_hip.h prints sizeof and every offsetof"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dojo_hip.h"\nint main(void) {\n    printf("sizeof %zu\\n", sizeof(DojoRiccati));\n'
                   + "".join('    printf("%s %%zu\\n", offsetof(DojoRiccati, %s));\n' % (f, f) for f in FIELDS) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True, timeout=120)
    out = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(api.DojoRiccati)
    assert [f for f, _ in api.DojoRiccati._fields_] == list(FIELDS)
    for f in FIELDS:
        assert int(out[f]) == getattr(api.DojoRiccati, f).offset, f
