"""Contact-data gradients through rollouts at the ABI (CPU tier): the five entry points are declared in include/dojo_hip.h, listed in
api.EXPORTED_SYMBOLS, exported by the built library, and the Julia shim names the host-pointer ones."""
import abi_checks
from dojo_amd import api

NAMES = ("dojo_set_contact_data", "dojo_get_contact_data", "dojo_rollout_data_record_dev", "dojo_rollout_data_adjoint_dev", "dojo_rollout_data_gradients")


def test_header_declares_the_entry_points():
    abi_checks.assert_declared(NAMES)
    hdr = abi_checks.text(abi_checks.HEADER)
    assert "src/gradients/contact.jl:1-55" in hdr and "examples/system_identification/utilities.jl:42-90" in hdr


def test_python_binding_lists_them():
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS, n
    for m in ("set_contact_data", "contact_data", "rollout_data_gradients"):
        assert hasattr(api.BatchedMechanism, m), m
    src = abi_checks.host_source("autograd")      # (importing it needs torch: the text is enough here)
    assert "def differentiable_data_rollout(" in src


def test_library_exports_them():
    abi_checks.assert_exported_and_bound(NAMES)


def test_julia_shim_names_the_host_entries():
    jl = abi_checks.text(abi_checks.JULIA_SHIM)
    assert "fn(:dojo_rollout_data_gradients)" in jl and "function rollout_data_gradients(" in jl
    assert "fn(:dojo_set_contact_data)" in jl and "function set_contact_data!(" in jl
