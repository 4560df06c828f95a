"""Forward-mode rollouts at the ABI (CPU tier): the two entry points are declared in include/dojo_hip.h, listed in api.EXPORTED_SYMBOLS and bound with
argument types, exported by the built library, and the Julia shim names the host-pointer one."""
import abi_checks
from dojo_amd import api

NAMES = ("dojo_rollout_tangent_dev", "dojo_rollout_tangents")


def test_header_declares_the_entry_points():
    abi_checks.assert_declared(NAMES)
    hdr = abi_checks.text(abi_checks.HEADER)
    # the documented contract: the recursion's failure rule, the NULL rules, the determinism statement, the memory formula
    for text in ("delta <- DZ_k[b] delta + DU_k[b] dU[k][b][t] + DC_k[b] dtheta[t]", "may be NULL", "bit-identical from run to run", "Memory of the call"):
        assert text in hdr, text


def test_python_binding_lists_them():
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS, n
    assert hasattr(api.BatchedMechanism, "rollout_tangents")


def test_library_exports_them():
    abi_checks.assert_exported_and_bound(NAMES)


def test_julia_shim_names_the_host_entry():
    jl = abi_checks.text(abi_checks.JULIA_SHIM)
    assert "fn(:dojo_rollout_tangents)" in jl and "function rollout_tangents(" in jl
