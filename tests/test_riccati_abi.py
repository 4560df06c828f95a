"""The Riccati backward pass at the ABI (CPU tier): the two entry points are declared in include/dojo_hip.h, listed in api.EXPORTED_SYMBOLS and bound with argument
types, exported by the built library, the Julia shim names the host-pointer one, and the ctypes mirror of `DojoRiccati` has the layout the C compiler gives the struct."""
import abi_checks
from dojo_amd import api

NAMES = ("dojo_riccati_dev", "dojo_riccati")
FIELDS = ("A", "Bm", "status", "lx", "lu", "lxx", "luu", "lux", "mu", "K", "kff", "fail", "dV", "Vx", "Vxx", "act_off", "na")


def test_header_declares_the_entry_points():
    abi_checks.assert_declared(NAMES)
    hdr = abi_checks.text(abi_checks.HEADER)
    # the documented contract: what it mirrors, the recursion's failure rules, the determinism statement, what is not part of it
    for text in ("IterativeLQR", "examples/trajectory_optimization", "fail <- k + 1", "A_k, B_k are NOT read", "bit-identical from run to run", "Not part of it"):
        assert text in hdr, text


def test_python_binding_lists_them():
    for n in NAMES:
        assert n in api.EXPORTED_SYMBOLS, n
    assert hasattr(api.BatchedMechanism, "riccati")
    ilqr = abi_checks.host_source("ilqr")      # (importing it needs torch: the text is enough here)
    for name in ("def linearize_rollout(gm, x0, U)", "def riccati(gm, A, Bm, lx, lu, lxx, luu, lux=None, mu=None, status=None, act_off=0, na=None, value=False)",
                 "class QuadraticCost", "def solve(gm, x0, U0, cost, iters, act_off=0, na=None"):
        assert name in ilqr, name


def test_library_exports_them():
    abi_checks.assert_exported_and_bound(NAMES)


def test_julia_shim_names_the_host_entry():
    jl = abi_checks.text(abi_checks.JULIA_SHIM)
    assert "fn(:dojo_riccati)" in jl and "function riccati(" in jl and "struct DojoRiccati" in jl


def test_ctypes_mirror_has_the_layout_of_the_c_struct():
    abi_checks.assert_mirror_layout("DojoRiccati", api.DojoRiccati, FIELDS)
