"""Closed-loop rollouts with a network policy at the ABI (CPU tier): the five entry points and the two records are declared in include/dojo_hip.h, the
entry points are listed in api.EXPORTED_SYMBOLS and exported by the built library, the Julia shim names the two host-pointer ones, the ctypes mirrors
of `DojoMlpPolicy` and `DojoMlpAdjoint` have the layout the C compiler gives the structs, and pack_mlp / unpack_mlp are each other's inverse in the
layout the header states."""
import re

import numpy as np
import pytest

import abi_checks
from dojo_amd import api

NAMES = ("dojo_rollout_mlp_dev", "dojo_rollout_mlp", "dojo_rollout_mlp_record_dev", "dojo_rollout_mlp_adjoint_dev", "dojo_rollout_mlp_gradients")
POLICY_FIELDS = ("theta", "mean", "scale", "U_ff", "per_env", "act_off", "n_layers", "width", "contact_forces", "contact_init", "reserved")
ADJOINT_FIELDS = ("DZ", "DU", "OBS", "ACT", "status", "z0", "Z", "M", "G", "G_u", "G_obs", "gtheta", "gU", "gz", "cot_space", "reserved")


def test_header_declares_the_entry_points():
    abi_checks.assert_declared(NAMES)
    hdr = abi_checks.text(abi_checks.HEADER)
    assert re.search(r"typedef\s+struct\s+DojoMlpPolicy\s*\{", hdr) and re.search(r"typedef\s+struct\s+DojoMlpAdjoint\s*\{", hdr)
    assert re.search(r"^#define\s+DOJO_MLP_MAX_LAYERS\s+%d\s*$" % api.MLP_MAX_LAYERS, hdr, re.M)
    assert "non-affine policies" not in hdr


def test_python_binding_lists_them():
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS, n
    for m in ("rollout_mlp", "rollout_mlp_gradients"):
        assert hasattr(api.BatchedMechanism, m), m
    src = abi_checks.host_source("autograd")      # (importing it needs torch: the text is enough here)
    assert "def differentiable_mlp_rollout(mech, z0, theta, widths, U_ff=None, steps=None, mean=None, scale=None, act_off=0)" in src


def test_library_exports_them():
    abi_checks.assert_exported_and_bound(NAMES)


def test_julia_shim_names_the_host_entries():
    jl = abi_checks.text(abi_checks.JULIA_SHIM)
    assert "fn(:dojo_rollout_mlp)" in jl and "function rollout_mlp(" in jl
    assert "fn(:dojo_rollout_mlp_gradients)" in jl and "function rollout_mlp_gradients(" in jl


@pytest.mark.parametrize("struct,fields", [("DojoMlpPolicy", POLICY_FIELDS), ("DojoMlpAdjoint", ADJOINT_FIELDS)])
def test_ctypes_mirrors_have_the_layout_of_the_c_structs(struct, fields):
    mirror = getattr(api, struct)
    abi_checks.assert_mirror_layout(struct, mirror, fields)
    if struct == "DojoMlpPolicy":
        assert mirror.width.size == 4 * (api.MLP_MAX_LAYERS + 1)


@pytest.mark.parametrize("lead", [(), (3,)])
@pytest.mark.parametrize("widths", [[4, 1], [2, 3, 1], [4, 17, 5, 1], [28, 64, 64, 16, 8]])
def test_pack_and_unpack_are_inverses(widths, lead):
    """theta is layer after layer W_l row-major, then b_l: checked entry by entry for the first and the last layer, and both round trips"""
    rng = np.random.default_rng(1)
    Ws = [rng.standard_normal(lead + (widths[l], widths[l - 1])) for l in range(1, len(widths))]
    bs = [rng.standard_normal(lead + (widths[l],)) for l in range(1, len(widths))]
    theta, w = api.pack_mlp(Ws, bs)
    P, nh = api.mlp_sizes(widths)
    assert w == widths and theta.shape == lead + (P,) and theta.flags["C_CONTIGUOUS"]
    assert P == sum(widths[l] * (widths[l - 1] + 1) for l in range(1, len(widths))) and nh == sum(widths[1:-1])
    n1 = widths[1] * widths[0]
    assert np.array_equal(theta[..., :n1], Ws[0].reshape(lead + (-1,))) and np.array_equal(theta[..., n1:n1 + widths[1]], bs[0])
    if widths[1] > 1:
        assert np.array_equal(theta[..., widths[0]], Ws[0][..., 1, 0])          # row-major: entry n_0 is W_1[1][0]
    assert np.array_equal(theta[..., P - widths[-1]:], bs[-1])
    W2, b2 = api.unpack_mlp(theta, widths)
    assert len(W2) == len(Ws) and all(np.array_equal(a, b) for a, b in zip(W2, Ws)) and all(np.array_equal(a, b) for a, b in zip(b2, bs))
    theta2, _ = api.pack_mlp(W2, b2)
    assert np.array_equal(theta2, theta)
    with pytest.raises(ValueError):
        api.unpack_mlp(theta[..., :-1], widths)
    with pytest.raises(ValueError):
        api.mlp_sizes([4, 3, 3, 3, 3, 1])
