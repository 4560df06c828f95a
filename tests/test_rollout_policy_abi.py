"""Closed-loop rollouts at the ABI (CPU tier): the two entry points are declared in include/dojo_hip.h, listed in api.EXPORTED_SYMBOLS, exported by the
built library, the Julia shim names the host-pointer one, and the ctypes mirror of `DojoPolicy` has the layout the C compiler gives the struct."""
import ctypes
import os
import re
import subprocess

from dojo_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dojo_rollout_policy_dev", "dojo_rollout_policy")
FIELDS = ("W", "bias", "mean", "scale", "U_ff", "per_env", "act_off", "na", "contact_forces", "contact_init", "reserved")


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dojo_hip.h")).read()
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(\s*DojoHandle\b" % n, hdr, re.M), n
    assert re.search(r"typedef\s+struct\s+DojoPolicy\s*\{", hdr)


def test_python_binding_lists_them():
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS, n
    assert hasattr(api.BatchedMechanism, "rollout_policy")
    src = open(os.path.join(ROOT, "dojo.jl_amd", "host", "dojo_amd", "envs.py")).read()      # (importing it needs torch: the text is enough here)
    assert "def rollout_policy(self, theta, horizon, mean=None, scale=None, U_ff=None)" in src


def test_library_exports_them():
    lib = ctypes.CDLL(os.path.join(ROOT, "dojo.jl_amd", "csrc", "libdojo_hip.so"))
    for n in NAMES:
        assert hasattr(lib, n), n


def test_julia_shim_names_the_host_entry():
    jl = open(os.path.join(ROOT, "dojo.jl_amd", "julia", "DojoHIP.jl")).read()
    assert "fn(:dojo_rollout_policy)" in jl and "function rollout_policy(" in jl


def test_ctypes_mirror_has_the_layout_of_the_c_struct(tmp_path):
    """a host-only C program compiled against include/dojo_hip.h prints sizeof and every offsetof"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dojo_hip.h"\nint main(void) {\n    printf("sizeof %zu\\n", sizeof(DojoPolicy));\n'
                   + "".join('    printf("%s %%zu\\n", offsetof(DojoPolicy, %s));\n' % (f, f) for f in FIELDS) + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True, timeout=120)
    out = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(api.DojoPolicy)
    assert [f for f, _ in api.DojoPolicy._fields_] == list(FIELDS)
    for f in FIELDS:
        assert int(out[f]) == getattr(api.DojoPolicy, f).offset, f
