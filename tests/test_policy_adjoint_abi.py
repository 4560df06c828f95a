"""Reverse mode through closed-loop rollouts at the ABI (CPU tier): the five entry points and the `DojoPolicyAdjoint` record are declared in
include/dojo_hip.h, the entry points are listed in api.EXPORTED_SYMBOLS and exported by the built library, the Julia shim names the host-pointer
one, and the ctypes mirror of `DojoPolicyAdjoint` has the layout the C compiler gives the struct."""
import abi_checks
from dojo_amd import api

NAMES = ("dojo_observation_jacobian_dev", "dojo_observation_jacobian", "dojo_rollout_policy_record_dev", "dojo_rollout_policy_adjoint_dev",
         "dojo_rollout_policy_gradients")
FIELDS = ("DZ", "DU", "OBS", "status", "z0", "Z", "M", "G", "G_u", "G_obs", "gW", "gbias", "gU", "gz", "cot_space", "reserved")


def test_header_declares_the_entry_points():
    abi_checks.assert_declared(NAMES)


def test_python_binding_lists_them():
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS, n
    for m in ("observation_jacobian", "rollout_policy_gradients"):
        assert hasattr(api.BatchedMechanism, m), m
    from dojo_amd import coords
    assert hasattr(coords, "dense_observation_jacobian")
    src = abi_checks.host_source("autograd")      # (importing it needs torch: the text is enough here)
    assert "def differentiable_policy_rollout(mech, z0, W, bias=None, U_ff=None, steps=None, mean=None, scale=None, act_off=0)" in src


def test_library_exports_them():
    abi_checks.assert_exported_and_bound(NAMES)


def test_julia_shim_names_the_host_entry():
    jl = abi_checks.text(abi_checks.JULIA_SHIM)
    assert "fn(:dojo_rollout_policy_gradients)" in jl and "function rollout_policy_gradients(" in jl


def test_ctypes_mirror_has_the_layout_of_the_c_struct():
    abi_checks.assert_mirror_layout("DojoPolicyAdjoint", api.DojoPolicyAdjoint, FIELDS)
