"""Reverse mode through closed-loop rollouts at the ABI (CPU tier): the five entry points and the `DojoPolicyAdjoint` record are declared in
include/dojo_hip.h, the entry points are listed in api.EXPORTED_SYMBOLS and exported by the built library, the Julia shim names the host-pointer
one, and the ctypes mirror of `DojoPolicyAdjoint` has the layout the C compiler gives the struct."""
import ctypes
import os
import re
import subprocess

from dojo_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dojo_observation_jacobian_dev", "dojo_observation_jacobian", "dojo_rollout_policy_record_dev", "dojo_rollout_policy_adjoint_dev",
         "dojo_rollout_policy_gradients")
FIELDS = ("DZ", "DU", "OBS", "status", "z0", "Z", "M", "G", "G_u", "G_obs", "gW", "gbias", "gU", "gz", "cot_space", "reserved")


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dojo_hip.h")).read()
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(\s*DojoHandle\b" % n, hdr, re.M), n
    assert re.search(r"typedef\s+struct\s+DojoPolicyAdjoint\s*\{", hdr)


def test_python_binding_lists_them():
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS, n
    for m in ("observation_jacobian", "rollout_policy_gradients"):
        assert hasattr(api.BatchedMechanism, m), m
    from dojo_amd import coords
    assert hasattr(coords, "dense_observation_jacobian")
    src = open(os.path.join(ROOT, "dojo.jl_amd", "host", "dojo_amd", "autograd.py")).read()      # (importing it needs torch: the text is enough here)
    assert "def differentiable_policy_rollout(mech, z0, W, bias=None, U_ff=None, steps=None, mean=None, scale=None, act_off=0)" in src


def test_library_exports_them():
    lib = ctypes.CDLL(os.path.join(ROOT, "dojo.jl_amd", "csrc", "libdojo_hip.so"))
    for n in NAMES:
        assert hasattr(lib, n), n


def test_julia_shim_names_the_host_entry():
    jl = open(os.path.join(ROOT, "dojo.jl_amd", "julia", "DojoHIP.jl")).read()
    assert "fn(:dojo_rollout_policy_gradients)" in jl and "function rollout_policy_gradients(" in jl


def test_ctypes_mirror_has_the_layout_of_the_c_struct(tmp_path):
    """a host-only C program compiled against include/dojo_hip.h prints sizeof and every offsetof"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dojo_hip.h"\nint main(void) {\n    printf("sizeof %zu\\n", sizeof(DojoPolicyAdjoint));\n'
                   + "".join('    printf("%s %%zu\\n", offsetof(DojoPolicyAdjoint, %s));\n' % (f, f) for f in FIELDS) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True, timeout=120)
    out = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(api.DojoPolicyAdjoint)
    assert [f for f, _ in api.DojoPolicyAdjoint._fields_] == list(FIELDS)
    for f in FIELDS:
        assert int(out[f]) == getattr(api.DojoPolicyAdjoint, f).offset, f
