"""Constrained iLQR at the ABI (CPU tier): the two entries are declared in the FOURTH public header, include/dojo_hip_constraints.h (which includes the third),
listed in api.CONSTRAINT_SYMBOLS and bound with the header's arity and kinds, exported by the built library; the ctypes mirror of `DojoStageConstraints` has the
layout the C compiler gives the struct; the Julia shim and dojo_amd/ilqr.py have the new names; the three older headers keep exactly their 74, 2 and 4 prototypes."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import abi_checks
from dojo_amd import api
from test_riccati_box_abi import prototypes

HEADER = os.path.join(abi_checks.ROOT, "include", "dojo_hip_constraints.h")
LIMITS = os.path.join(abi_checks.ROOT, "include", "dojo_hip_limits.h")
TRAJOPT = os.path.join(abi_checks.ROOT, "include", "dojo_hip_trajopt.h")
NAMES = ("dojo_riccati_al_dev", "dojo_riccati_al")
FIELDS = ("Cx", "Cu", "w", "y", "nc", "shared")


def test_new_header_declares_exactly_the_two_entry_points():
    hdr = abi_checks.text(HEADER)
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(\s*DojoHandle\b" % n, hdr, re.M), n
    assert tuple(prototypes(HEADER)) == NAMES
    assert '#include "dojo_hip_limits.h"' in hdr
    assert re.search(r"typedef\s+struct\s+DojoStageConstraints\s*\{\s*const\s+void\s*\*\s*Cx\s*,\s*\*\s*Cu\s*,\s*\*\s*w\s*,\s*\*\s*y\s*;\s*int32_t\s+nc\s*,\s*shared\s*;\s*\}\s*DojoStageConstraints\s*;", hdr)
    # the documented contract: the recursion, the rows that are not loaded, determinism, the bits of the other entries, the refusals, what is not part of it
    for text in ("G_k' diag(w) G_k", "G_k' y", "w[k][b][i] == 0 and y[k][b][i] == 0", "NOT LOADED", "ALSO at a step with status != 0", "lim = NULL: no control limits",
                 "M = J + sum lambda c + 1/2 sum w c^2", "bit-identical from run", "dojo_riccati_box_dev's bit for bit", "dojo_riccati_dev's", "DOJO_ERR_UNSUPPORTED",
                 "NULL con, nc < 0, nc > 0", "NULL U with non-NULL lim", "w < 0 and NaN in w or y", "No atomics",
                 "Not part of it: second-order constraint terms, constraints evaluated on the device, per-row penalties", "a warm start of the"):
        assert text in hdr, text


def test_older_headers_keep_their_prototypes():
    assert len(abi_checks.header_prototypes()) == len(api.EXPORTED_SYMBOLS) == 74
    assert tuple(prototypes(TRAJOPT)) == tuple(api.TRAJOPT_SYMBOLS) and len(api.TRAJOPT_SYMBOLS) == 2
    assert tuple(prototypes(LIMITS)) == tuple(api.LIMITS_SYMBOLS) and len(api.LIMITS_SYMBOLS) == 4
    for path in (abi_checks.HEADER, TRAJOPT, LIMITS):
        assert not any(re.search(r"\b%s\s*\(" % n, abi_checks.text(path)) for n in NAMES) and "DojoStageConstraints" not in abi_checks.text(path)
    assert "dojo_hip_constraints.h" in abi_checks.text(os.path.join("dojo.jl_amd", "csrc", "dojo_riccati.hpp"))


def test_python_binding_lists_and_binds_them_with_the_headers_kinds():
    assert tuple(api.CONSTRAINT_SYMBOLS) == NAMES
    assert not set(NAMES) & (set(api.EXPORTED_SYMBOLS) | set(api.TRAJOPT_SYMBOLS) | set(api.LIMITS_SYMBOLS))
    assert hasattr(api.BatchedMechanism, "riccati_al")
    protos = prototypes(HEADER)
    for n in NAMES:
        f = getattr(api.lib(), n)
        assert f.restype is C.c_int and list(f.argtypes) == protos[n], n
    assert api.lib().dojo_riccati_al_dev.argtypes == [C.c_void_p, C.c_int32] + [C.c_void_p] * 7
    assert api.lib().dojo_riccati_al.argtypes == [C.c_void_p, C.c_int32] + [C.c_void_p] * 6


def test_library_exports_them():
    built = C.CDLL(abi_checks.LIBRARY)
    for n in NAMES:
        assert hasattr(built, n), n


def test_build_sees_the_new_header():
    src = abi_checks.text("__graft_entry__.py")
    assert src.count('"dojo_hip_constraints.h"') == 2
    assert '#include "../../include/dojo_hip_constraints.h"' in abi_checks.text(os.path.join("dojo.jl_amd", "csrc", "dojo_hip.hip"))


def test_ctypes_mirror_has_the_layout_of_the_c_struct():
    assert [f[0] for f in api.DojoStageConstraints._fields_] == list(FIELDS)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "dojo_hip_constraints.h"\nint main(void) {\n    printf("%zu\\n", sizeof(DojoStageConstraints));\n'
                    + "".join('    printf("%%zu\\n", offsetof(DojoStageConstraints, %s));\n' % m for m in FIELDS)
                    + '    printf("%zu\\n%zu\\n%zu\\n", sizeof(DojoRiccati), sizeof(DojoTracking), sizeof(DojoControlLimits));\n    return 0;\n}\n')
        subprocess.run(["cc", "-I" + os.path.dirname(HEADER), src, "-o", exe], check=True, capture_output=True, text=True, timeout=120)
        vals = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    n = len(FIELDS)
    assert abi_checks.mirror_layout(api.DojoStageConstraints) == (vals[0], list(zip(FIELDS, vals[1:1 + n])))
    assert vals[1 + n:] == [C.sizeof(api.DojoRiccati), C.sizeof(api.DojoTracking), C.sizeof(api.DojoControlLimits)]     # (the new header brings the older structs along unchanged)


def test_julia_shim_has_the_new_names():
    jl = abi_checks.text(abi_checks.JULIA_SHIM)
    for text in ("struct DojoStageConstraints", "nc::Int32; shared::Int32", "fn(:dojo_riccati_al)", "function riccati_al("):
        assert text in jl, text


def test_ilqr_has_the_new_functions_and_keeps_the_old_signatures():
    src = abi_checks.host_source("ilqr")
    for name in ("def riccati_al(gm, A, Bm, lx, lu, lxx, luu, Cx, w, y, Cu=None, shared=False, U=None, lo=None, hi=None, lux=None, mu=None, status=None, act_off=0, na=None,",
                 "def solve_constrained(gm, x0, U0, cost, constraints, iters, outer, lo=None, hi=None, rho0=1.0, rho_scale=10.0, rho_max=1e8,",
                 "class GoalConstraint:", "def __init__(self, x_goal, rows=None):", "class StateBounds:", "def __init__(self, lo, hi, rows=None):",
                 "def riccati_box(gm, A, Bm, lx, lu, lxx, luu, U, lo, hi,", "def solve_limited(gm, x0, U0, cost, iters, lo, hi,", "def _solve(",
                 "def riccati(gm, A, Bm, lx, lu, lxx, luu, lux=None, mu=None, status=None, act_off=0, na=None, value=False)",
                 "def solve(gm, x0, U0, cost, iters, act_off=0, na=None"):
        assert name in src, name
    assert "dojo_hip_constraints.h" in src
    sig = inspect.signature(api.BatchedMechanism.riccati_al)
    assert list(sig.parameters)[:10] == ["self", "A", "Bm", "lx", "lu", "lxx", "luu", "Cx", "w", "y"]
