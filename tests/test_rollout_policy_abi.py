"""Closed-loop rollouts at the ABI (CPU tier): the two entry points are declared in include/dojo_hip.h, listed in api.EXPORTED_SYMBOLS, exported by the
built library, the Julia shim names the host-pointer one, and the ctypes mirror of `DojoPolicy` has the layout the C compiler gives the struct."""
import abi_checks
from dojo_amd import api

NAMES = ("dojo_rollout_policy_dev", "dojo_rollout_policy")
FIELDS = ("W", "bias", "mean", "scale", "U_ff", "per_env", "act_off", "na", "contact_forces", "contact_init", "reserved")


def test_header_declares_the_entry_points():
    abi_checks.assert_declared(NAMES)


def test_python_binding_lists_them():
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS, n
    assert hasattr(api.BatchedMechanism, "rollout_policy")
    src = abi_checks.host_source("envs")      # (importing it needs torch: the text is enough here)
    assert "def rollout_policy(self, theta, horizon, mean=None, scale=None, U_ff=None)" in src


def test_library_exports_them():
    abi_checks.assert_exported_and_bound(NAMES)


def test_julia_shim_names_the_host_entry():
    jl = abi_checks.text(abi_checks.JULIA_SHIM)
    assert "fn(:dojo_rollout_policy)" in jl and "function rollout_policy(" in jl


def test_ctypes_mirror_has_the_layout_of_the_c_struct():
    abi_checks.assert_mirror_layout("DojoPolicy", api.DojoPolicy, FIELDS)
