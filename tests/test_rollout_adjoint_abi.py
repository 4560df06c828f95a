"""Reverse-mode rollouts at the ABI (CPU tier): the three entry points are declared in include/dojo_hip.h, listed in
api.EXPORTED_SYMBOLS, exported by the built library, and the Julia shim names the host-pointer one."""
import abi_checks
from dojo_amd import api

NAMES = ("dojo_rollout_record_dev", "dojo_rollout_adjoint_dev", "dojo_rollout_gradients")


def test_header_declares_the_entry_points():
    abi_checks.assert_declared(NAMES)


def test_python_binding_lists_them():
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS, n
    assert hasattr(api.BatchedMechanism, "rollout_gradients")
    src = abi_checks.host_source("autograd")      # (importing it needs torch: the text is enough here)
    assert "def differentiable_rollout(" in src


def test_library_exports_them():
    abi_checks.assert_exported_and_bound(NAMES)


def test_julia_shim_names_the_host_entry():
    jl = abi_checks.text(abi_checks.JULIA_SHIM)
    assert "fn(:dojo_rollout_gradients)" in jl and "function rollout_gradients(" in jl
