"""Control-limited iLQR at the ABI (CPU tier): the four entries are declared in the THIRD public header, include/dojo_hip_limits.h (which includes the second),
listed in api.LIMITS_SYMBOLS and bound with the header's arity and kinds, exported by the built library; the ctypes mirror of `DojoControlLimits` has the layout
the C compiler gives the struct; the Julia shim and dojo_amd/ilqr.py have the new names; the two older headers keep exactly their 74 and 2 prototypes."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import abi_checks
from dojo_amd import api

HEADER = os.path.join(abi_checks.ROOT, "include", "dojo_hip_limits.h")
TRAJOPT = os.path.join(abi_checks.ROOT, "include", "dojo_hip_trajopt.h")
NAMES = ("dojo_riccati_box_dev", "dojo_riccati_box", "dojo_rollout_minimal_box_dev", "dojo_rollout_minimal_box")


def prototypes(path):
    """name -> [ctypes kind of every parameter], of the `int dojo_*(..);` prototypes of a header (comments removed)"""
    code = re.sub(r"/\*.*?\*/", " ", abi_checks.text(path), flags=re.S)
    return {name: [abi_checks._kind(p) for p in " ".join(params.split()).split(",")]
            for name, params in re.findall(r"^\s*int\s+(dojo_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", code, flags=re.M)}


def test_new_header_declares_exactly_the_four_entry_points():
    hdr = abi_checks.text(HEADER)
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(\s*DojoHandle\b" % n, hdr, re.M), n
    assert tuple(prototypes(HEADER)) == NAMES
    assert '#include "dojo_hip_trajopt.h"' in hdr
    assert re.search(r"typedef\s+struct\s+DojoControlLimits\s*\{\s*const\s+void\s*\*\s*lo\s*,\s*\*\s*hi\s*;\s*\}\s*DojoControlLimits\s*;", hdr)
    # the documented contract: the recursion, the solver, the determinism statement, the failure codes, the refusals, what is not part of it
    for text in ("argmin_x", "K[clamped rows] = 0", "projected Newton", "at most 40 trials", "64 iterations", "fail[b] = -(k + 1)", "fail[b] = k + 1",
                 "bit-identical from run", "DOJO_ERR_UNSUPPORTED", "NULL lim or NULL U", "refuses lo > hi and NaN", "rounding is monotone",
                 "Not part of it: state constraints, time-varying limits, a warm start", "limits on inputs that are not driven"):
        assert text in hdr, text


def test_older_headers_keep_their_prototypes_and_point_here():
    assert len(abi_checks.header_prototypes()) == len(api.EXPORTED_SYMBOLS) == 74
    assert tuple(prototypes(TRAJOPT)) == tuple(api.TRAJOPT_SYMBOLS) and len(api.TRAJOPT_SYMBOLS) == 2
    first, second = abi_checks.text(abi_checks.HEADER), abi_checks.text(TRAJOPT)
    assert "dojo_hip_limits.h" in first and "dojo_hip_limits.h" in second
    assert not any(n in first for n in NAMES) and not any(re.search(r"\b%s\s*\(" % n, second) for n in NAMES)
    assert "dojo_hip_limits.h" in abi_checks.text(os.path.join("dojo.jl_amd", "csrc", "dojo_riccati.hpp"))


def test_python_binding_lists_and_binds_them_with_the_headers_kinds():
    assert tuple(api.LIMITS_SYMBOLS) == NAMES
    assert not set(NAMES) & set(api.EXPORTED_SYMBOLS) and not set(NAMES) & set(api.TRAJOPT_SYMBOLS)
    assert hasattr(api.BatchedMechanism, "riccati_box") and hasattr(api.BatchedMechanism, "rollout_minimal_box")
    protos = prototypes(HEADER)
    for n in NAMES:
        f = getattr(api.lib(), n)
        assert f.restype is C.c_int and list(f.argtypes) == protos[n], n
    assert api.lib().dojo_riccati_box_dev.argtypes == [C.c_void_p, C.c_int32] + [C.c_void_p] * 6


def test_library_exports_them():
    built = C.CDLL(abi_checks.LIBRARY)
    for n in NAMES:
        assert hasattr(built, n), n


def test_build_sees_the_new_header():
    src = abi_checks.text("__graft_entry__.py")
    assert src.count('"dojo_hip_limits.h"') == 2 and src.count('"dojo_hip_trajopt.h"') == 2


def test_ctypes_mirror_has_the_layout_of_the_c_struct():
    fields = ("lo", "hi")
    assert [f[0] for f in api.DojoControlLimits._fields_] == list(fields)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "dojo_hip_limits.h"\nint main(void) {\n    printf("%zu\\n", sizeof(DojoControlLimits));\n'
                    + "".join('    printf("%%zu\\n", offsetof(DojoControlLimits, %s));\n' % m for m in fields)
                    + '    printf("%zu\\n%zu\\n", sizeof(DojoRiccati), sizeof(DojoTracking));\n    return 0;\n}\n')
        subprocess.run(["cc", "-I" + os.path.dirname(HEADER), src, "-o", exe], check=True, capture_output=True, text=True, timeout=120)
        vals = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert abi_checks.mirror_layout(api.DojoControlLimits) == (vals[0], list(zip(fields, vals[1:3])))
    assert vals[3:] == [C.sizeof(api.DojoRiccati), C.sizeof(api.DojoTracking)]          # (the new header brings the older structs along unchanged)


def test_julia_shim_has_the_new_names():
    jl = abi_checks.text(abi_checks.JULIA_SHIM)
    for text in ("struct DojoControlLimits", "fn(:dojo_riccati_box)", "function riccati_box(", "fn(:dojo_rollout_minimal_box)", "function rollout_minimal_box("):
        assert text in jl, text


def test_ilqr_has_the_new_functions_and_keeps_the_old_signatures():
    ilqr = abi_checks.host_source("ilqr")
    for name in ("def riccati_box(gm, A, Bm, lx, lu, lxx, luu, U, lo, hi,", "def rollout_minimal_box(gm, x0, Ubar, lo, hi,",
                 "def forward_pass_box(gm, Xbar, Ubar, K, kff, a, act_off, na, lo, hi)", "def solve_limited(gm, x0, U0, cost, iters, lo, hi,", "def _solve(",
                 "def riccati(gm, A, Bm, lx, lu, lxx, luu, lux=None, mu=None, status=None, act_off=0, na=None, value=False)",
                 "def solve(gm, x0, U0, cost, iters, act_off=0, na=None", "mu_shrink=0.1, fused=False):"):
        assert name in ilqr, name
    assert "dojo_hip_limits.h" in ilqr
