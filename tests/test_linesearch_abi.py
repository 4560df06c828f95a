"""The side-by-side line search at the ABI (CPU tier): the four entries are declared in the FIFTH public header, include/dojo_hip_linesearch.h (which includes the
fourth), listed in api.LINESEARCH_SYMBOLS and bound with the header's arity and kinds, exported by the built library; the ctypes mirrors of `DojoQuadraticCost`
and `DojoLineSearch` have the layout the C compiler gives the structs; the Julia shim and dojo_amd/ilqr.py have the new names; the four older headers keep
exactly their 74, 2, 4 and 2 prototypes."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import abi_checks
from dojo_amd import api
from test_riccati_box_abi import prototypes

HEADER = os.path.join(abi_checks.ROOT, "include", "dojo_hip_linesearch.h")
CONSTRAINTS = os.path.join(abi_checks.ROOT, "include", "dojo_hip_constraints.h")
LIMITS = os.path.join(abi_checks.ROOT, "include", "dojo_hip_limits.h")
TRAJOPT = os.path.join(abi_checks.ROOT, "include", "dojo_hip_trajopt.h")
NAMES = ("dojo_rollout_minimal_fan_dev", "dojo_rollout_minimal_fan", "dojo_linesearch_select_dev", "dojo_linesearch_select")
COST_FIELDS = ("Q", "R", "Qf", "goal", "goal_per_problem")
LS_FIELDS = ("X", "U", "status", "alpha", "dV", "ok", "Xcur", "Ucur", "J0", "J_trial", "J_cur", "J_acc", "choice", "alpha_acc", "X_new", "U_new", "c1", "act_off", "na")


def test_new_header_declares_exactly_the_four_entry_points():
    hdr = abi_checks.text(HEADER)
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(\s*DojoHandle\b" % n, hdr, re.M), n
    assert tuple(prototypes(HEADER)) == NAMES
    assert '#include "dojo_hip_constraints.h"' in hdr
    assert re.search(r"typedef\s+struct\s+DojoQuadraticCost\s*\{\s*const\s+void\s*\*\s*Q\s*,\s*\*\s*R\s*,\s*\*\s*Qf\s*,\s*\*\s*goal\s*;\s*int32_t\s+goal_per_problem\s*;\s*\}\s*DojoQuadraticCost\s*;", hdr)
    assert re.search(r"typedef\s+struct\s+DojoLineSearch\s*\{", hdr)
    # the documented contract: the layout, the law, the bits, the cost, the rule, the outputs, determinism, the refusals, what is not part of it
    for text in ("e = tr P + p", "p = e mod P", "alpha [T][P]", "dojo_rollout_minimal_box_dev", "bit for bit", "a group may begin and end inside a trial",
                 "A or Bm given", "B mod T != 0", "the cost values are double", "OUTPUT with a cost, INPUT without", "the FIRST acceptable tr in ascending order",
                 "J_tr is not NaN", "alpha_acc = 0", "Every element of every non-NULL output is written", "No atomics", "bit-identical from run", "T > 64",
                 "NULL J0 without a cost", "c1 not finite", "Not part of it: constraints in the side-by-side driver"):
        assert text in hdr, text


def test_older_headers_keep_their_prototypes():
    assert len(abi_checks.header_prototypes()) == len(api.EXPORTED_SYMBOLS) == 74
    assert tuple(prototypes(TRAJOPT)) == tuple(api.TRAJOPT_SYMBOLS) and len(api.TRAJOPT_SYMBOLS) == 2
    assert tuple(prototypes(LIMITS)) == tuple(api.LIMITS_SYMBOLS) and len(api.LIMITS_SYMBOLS) == 4
    assert tuple(prototypes(CONSTRAINTS)) == tuple(api.CONSTRAINT_SYMBOLS) and len(api.CONSTRAINT_SYMBOLS) == 2
    for path in (abi_checks.HEADER, TRAJOPT, LIMITS, CONSTRAINTS):
        older = abi_checks.text(path)
        assert not any(re.search(r"\b%s\b" % n, older) for n in NAMES) and "DojoLineSearch" not in older and "DojoQuadraticCost" not in older
        assert "dojo_hip_linesearch.h" in older          # ... and point here
    assert "dojo_hip_linesearch.h" in abi_checks.text(os.path.join("dojo.jl_amd", "csrc", "dojo_linesearch.hpp"))
    assert "dojo_hip_linesearch.h" in abi_checks.text(os.path.join("dojo.jl_amd", "csrc", "dojo_tracking.hpp"))


def test_python_binding_lists_and_binds_them_with_the_headers_kinds():
    assert tuple(api.LINESEARCH_SYMBOLS) == NAMES
    assert not set(NAMES) & (set(api.EXPORTED_SYMBOLS) | set(api.TRAJOPT_SYMBOLS) | set(api.LIMITS_SYMBOLS) | set(api.CONSTRAINT_SYMBOLS))
    assert hasattr(api.BatchedMechanism, "rollout_minimal_fan") and hasattr(api.BatchedMechanism, "linesearch_select")
    protos = prototypes(HEADER)
    for n in NAMES:
        f = getattr(api.lib(), n)
        assert f.restype is C.c_int and list(f.argtypes) == protos[n], n
    assert api.lib().dojo_rollout_minimal_fan_dev.argtypes == [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 3
    assert api.lib().dojo_linesearch_select.argtypes == [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 2


def test_library_exports_them():
    built = C.CDLL(abi_checks.LIBRARY)
    for n in NAMES:
        assert hasattr(built, n), n


def test_build_sees_the_new_header():
    src = abi_checks.text("__graft_entry__.py")
    for h in ("dojo_hip.h", "dojo_hip_trajopt.h", "dojo_hip_limits.h", "dojo_hip_constraints.h", "dojo_hip_linesearch.h"):
        assert src.count('"%s"' % h) == 2, h
    assert '#include "../../include/dojo_hip_linesearch.h"' in abi_checks.text(os.path.join("dojo.jl_amd", "csrc", "dojo_hip.hip"))


def test_ctypes_mirrors_have_the_layout_of_the_c_structs():
    assert [f[0] for f in api.DojoQuadraticCost._fields_] == list(COST_FIELDS) and [f[0] for f in api.DojoLineSearch._fields_] == list(LS_FIELDS)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "dojo_hip_linesearch.h"\nint main(void) {\n'
                    + "".join('    printf("%%zu\\n", sizeof(%s));\n' % s + "".join('    printf("%%zu\\n", offsetof(%s, %s));\n' % (s, m) for m in fields)
                              for s, fields in (("DojoQuadraticCost", COST_FIELDS), ("DojoLineSearch", LS_FIELDS)))
                    + '    printf("%zu\\n%zu\\n%zu\\n%zu\\n", sizeof(DojoRiccati), sizeof(DojoTracking), sizeof(DojoControlLimits), sizeof(DojoStageConstraints));\n    return 0;\n}\n')
        subprocess.run(["cc", "-I" + os.path.dirname(HEADER), src, "-o", exe], check=True, capture_output=True, text=True, timeout=120)
        vals = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    nc, nl = len(COST_FIELDS), len(LS_FIELDS)
    assert abi_checks.mirror_layout(api.DojoQuadraticCost) == (vals[0], list(zip(COST_FIELDS, vals[1:1 + nc])))
    assert abi_checks.mirror_layout(api.DojoLineSearch) == (vals[1 + nc], list(zip(LS_FIELDS, vals[2 + nc:2 + nc + nl])))
    # (the new header brings the older structs along unchanged)
    assert vals[2 + nc + nl:] == [C.sizeof(api.DojoRiccati), C.sizeof(api.DojoTracking), C.sizeof(api.DojoControlLimits), C.sizeof(api.DojoStageConstraints)]


def test_julia_shim_has_the_new_names():
    jl = abi_checks.text(abi_checks.JULIA_SHIM)
    for text in ("struct DojoQuadraticCost", "struct DojoLineSearch", "goal_per_problem::Int32", "c1::Float64; act_off::Int32; na::Int32", "fn(:dojo_rollout_minimal_fan)",
                 "fn(:dojo_linesearch_select)", "function rollout_minimal_fan(", "function linesearch_select("):
        assert text in jl, text


def test_ilqr_has_the_new_functions_and_keeps_the_old_signatures():
    src = abi_checks.host_source("ilqr")
    for name in ("def rollout_minimal_fan(gm_trials, T, x0, Ubar, Xbar, K, kff, alpha, lo=None, hi=None, act_off=0, na=None)", "def linesearch_select(gm_trials, T, ",
                 "def solve_side_by_side(gm, gm_trials, x0, U0, cost, iters, lo=None, hi=None,",
                 "def riccati_al(gm, A, Bm, lx, lu, lxx, luu, Cx, w, y, Cu=None, shared=False, U=None, lo=None, hi=None, lux=None, mu=None, status=None, act_off=0, na=None,",
                 "def solve_constrained(gm, x0, U0, cost, constraints, iters, outer, lo=None, hi=None, rho0=1.0, rho_scale=10.0, rho_max=1e8,",
                 "def riccati_box(gm, A, Bm, lx, lu, lxx, luu, U, lo, hi,", "def solve_limited(gm, x0, U0, cost, iters, lo, hi,", "def _solve(",
                 "def _solve(gm, x0, U0, cost, iters, act_off, na, c1, alphas, mu_init, mu_min, mu_grow, mu_shrink, fused, limits, al=None):",
                 "def rollout_minimal(gm, x0, Ubar, Xbar=None, K=None, kff=None, alpha=None, act_off=0, na=None, jacobians=False)",
                 "def riccati(gm, A, Bm, lx, lu, lxx, luu, lux=None, mu=None, status=None, act_off=0, na=None, value=False)",
                 "def solve(gm, x0, U0, cost, iters, act_off=0, na=None", "mu_shrink=0.1, fused=False):"):
        assert name in src, name
    assert "dojo_hip_linesearch.h" in src
    assert "running the step lengths of a line search side by side, kinematic" not in src          # the "Not here" sentence no longer lists it
    assert list(inspect.signature(api.BatchedMechanism.rollout_minimal_fan).parameters)[:3] == ["self", "T", "x0"]
    assert list(inspect.signature(api.BatchedMechanism.linesearch_select).parameters)[:8] == ["self", "T", "X", "U", "alpha", "dV", "Xcur", "Ucur"]
