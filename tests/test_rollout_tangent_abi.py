"""Forward-mode rollouts at the ABI (CPU tier): the two entry points are declared in include/dojo_hip.h, listed in api.EXPORTED_SYMBOLS and bound with
argument types, exported by the built library, and the Julia shim names the host-pointer one."""
import ctypes
import os
import re

from dojo_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dojo_rollout_tangent_dev", "dojo_rollout_tangents")


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dojo_hip.h")).read()
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(\s*DojoHandle\b" % n, hdr, re.M), n
    # the documented contract: the recursion's failure rule, the NULL rules, the determinism statement, the memory formula
    for text in ("delta <- DZ_k[b] delta + DU_k[b] dU[k][b][t] + DC_k[b] dtheta[t]", "may be NULL", "bit-identical from run to run", "Memory of the call"):
        assert text in hdr, text


def test_python_binding_lists_them():
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS, n
    assert hasattr(api.BatchedMechanism, "rollout_tangents")
    src = open(os.path.join(ROOT, "dojo.jl_amd", "host", "dojo_amd", "api.py")).read()
    for n in NAMES:
        assert "L.%s.argtypes" % n in src, n


def test_library_exports_them():
    lib = ctypes.CDLL(os.path.join(ROOT, "dojo.jl_amd", "csrc", "libdojo_hip.so"))
    for n in NAMES:
        assert hasattr(lib, n), n
    L = api.lib()
    assert len(L.dojo_rollout_tangent_dev.argtypes) == 14 and len(L.dojo_rollout_tangents.argtypes) == 12


def test_julia_shim_names_the_host_entry():
    jl = open(os.path.join(ROOT, "dojo.jl_amd", "julia", "DojoHIP.jl")).read()
    assert "fn(:dojo_rollout_tangents)" in jl and "function rollout_tangents(" in jl
