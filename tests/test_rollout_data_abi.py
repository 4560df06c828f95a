"""Contact-data gradients through rollouts at the ABI (CPU tier): the five entry points are declared in include/dojo_hip.h, listed in
api.EXPORTED_SYMBOLS, exported by the built library, and the Julia shim names the host-pointer ones."""
import ctypes
import os
import re

from dojo_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dojo_set_contact_data", "dojo_get_contact_data", "dojo_rollout_data_record_dev", "dojo_rollout_data_adjoint_dev", "dojo_rollout_data_gradients")


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dojo_hip.h")).read()
    for n in NAMES:
        assert re.search(r"^int\s+%s\s*\(\s*DojoHandle\b" % n, hdr, re.M), n
    assert "src/gradients/contact.jl:1-55" in hdr and "examples/system_identification/utilities.jl:42-90" in hdr


def test_python_binding_lists_them():
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS, n
    for m in ("set_contact_data", "contact_data", "rollout_data_gradients"):
        assert hasattr(api.BatchedMechanism, m), m
    src = open(os.path.join(ROOT, "dojo.jl_amd", "host", "dojo_amd", "autograd.py")).read()      # (importing it needs torch: the text is enough here)
    assert "def differentiable_data_rollout(" in src


def test_library_exports_them():
    lib = ctypes.CDLL(os.path.join(ROOT, "dojo.jl_amd", "csrc", "libdojo_hip.so"))
    for n in NAMES:
        assert hasattr(lib, n), n


def test_julia_shim_names_the_host_entries():
    jl = open(os.path.join(ROOT, "dojo.jl_amd", "julia", "DojoHIP.jl")).read()
    assert "fn(:dojo_rollout_data_gradients)" in jl and "function rollout_data_gradients(" in jl
    assert "fn(:dojo_set_contact_data)" in jl and "function set_contact_data!(" in jl
