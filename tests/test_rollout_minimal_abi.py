"""The rollout in minimal coordinates at the ABI (CPU tier): the two entries are declared in the SECOND public header, include/dojo_hip_trajopt.h, listed in
api.TRAJOPT_SYMBOLS and bound with the prototype's arity, exported by the built library, the Julia shim names the host-pointer one, dojo_amd/ilqr.py has the
three new functions, and the ctypes mirror of `DojoTracking` has the layout the C compiler gives the struct."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import abi_checks
from dojo_amd import api

HEADER = os.path.join(abi_checks.ROOT, "include", "dojo_hip_trajopt.h")
NAMES = ("dojo_rollout_minimal_dev", "dojo_rollout_minimal")
FIELDS = ("x0", "Ubar", "Xbar", "K", "kff", "alpha", "X", "U_out", "status", "A", "Bm", "act_off", "na")


def prototypes():
    """name -> number of parameters, of the `int dojo_*(..);` prototypes of the new header (comments removed)"""
    code = re.sub(r"/\*.*?\*/", " ", abi_checks.text(HEADER), flags=re.S)
    return {name: len(params.split(",")) for name, params in re.findall(r"^\s*int\s+(dojo_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", code, flags=re.M)}


def c_layout(struct_name, members):
    """(sizeof, [(member, offsetof), ..]) of a struct of the NEW header: a host-only C program compiled against it prints them (abi_checks.c_layout includes the
    first header alone)"""
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "dojo_hip_trajopt.h"\nint main(void) {\n    printf("%%zu\\n", sizeof(%s));\n' % struct_name
                    + "".join('    printf("%%zu\\n", offsetof(%s, %s));\n' % (struct_name, m) for m in members) + "    return 0;\n}\n")
        subprocess.run(["cc", "-I" + os.path.dirname(HEADER), src, "-o", exe], check=True, capture_output=True, text=True, timeout=120)
        vals = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    return vals[0], list(zip(members, vals[1:]))


def test_new_header_declares_the_entry_points():
    hdr = abi_checks.text(HEADER)
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(\s*DojoHandle\b" % n, hdr, re.M), n
    assert set(prototypes()) == set(NAMES)
    assert '#include "dojo_hip.h"' in hdr
    # the documented contract: the law, the determinism statement, the refusals, what is not part of it
    for text in ("fma(alpha[b], kff[k][b][i]", "from the ROUNDED X[k]", "bit-identical from run", "exactly one of A, Bm given", "Not part of it", "dojo_minimal_gradients_dev"):
        assert text in hdr, text


def test_first_header_points_to_the_new_one_and_keeps_its_entries():
    first = abi_checks.text(abi_checks.HEADER)
    assert "dojo_hip_trajopt.h" in first and "the forward pass as one fused call" not in first
    assert not any(n in first for n in NAMES)
    assert len(abi_checks.header_prototypes()) == len(api.EXPORTED_SYMBOLS)


def test_python_binding_lists_and_binds_them():
    assert tuple(api.TRAJOPT_SYMBOLS) == NAMES
    assert not set(NAMES) & set(api.EXPORTED_SYMBOLS)
    assert hasattr(api.BatchedMechanism, "rollout_minimal")
    arity = prototypes()
    for n in NAMES:
        f = getattr(api.lib(), n)
        assert f.restype is C.c_int and len(f.argtypes) == arity[n], n
    assert api.lib().dojo_rollout_minimal_dev.argtypes == [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]


def test_library_exports_them():
    built = C.CDLL(abi_checks.LIBRARY)
    for n in NAMES:
        assert hasattr(built, n), n


def test_build_stamp_sees_the_new_header():
    src = abi_checks.text("__graft_entry__.py")
    assert src.count('"dojo_hip_trajopt.h"') == 2


def test_julia_shim_names_the_host_entry():
    jl = abi_checks.text(abi_checks.JULIA_SHIM)
    assert "fn(:dojo_rollout_minimal)" in jl and "function rollout_minimal(" in jl and "struct DojoTracking" in jl


def test_ilqr_has_the_three_new_functions_and_keeps_the_old_signatures():
    ilqr = abi_checks.host_source("ilqr")
    for name in ("def rollout_minimal(gm, x0, Ubar, Xbar=None, K=None, kff=None, alpha=None, act_off=0, na=None, jacobians=False)",
                 "def linearize_rollout_fused(gm, x0, U)", "def forward_pass_fused(gm, Xbar, Ubar, K, kff, alpha, act_off, na)",
                 "def linearize_rollout(gm, x0, U)", "def forward_pass(gm, Xbar, Ubar, K, kff, a, act_off, na)", "mu_shrink=0.1, fused=False):"):
        assert name in ilqr, name
    assert "the forward pass as one fused call" not in ilqr


def test_ctypes_mirror_has_the_layout_of_the_c_struct():
    assert re.search(r"typedef\s+struct\s+DojoTracking\s*\{", abi_checks.text(HEADER))
    assert [f[0] for f in api.DojoTracking._fields_] == list(FIELDS)
    assert abi_checks.mirror_layout(api.DojoTracking) == c_layout("DojoTracking", FIELDS)
