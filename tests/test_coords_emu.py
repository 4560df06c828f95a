"""The coordinate templates of dojo.jl_amd/csrc/dojo_coords.hpp on the host (tests/emu/coords_emu.cpp: joint_min2max / joint_max2min for double and
Dual<24>, compiled with g++) against the C++ oracle, for every joint prototype and on the edge inputs of tests/fd_coords.py: rotations at 0, on either
side of the series switches of aa2qS (|r| = 1e-6) and rotvecS (a rotation of about 4e-6), and beyond pi.  The oracle has no series (it branches on
mag > 0), so it is an independent reference at the switches; its Jacobians are Richardson-extrapolated central differences of its maps.

This tier pins the branches and the dual arithmetic without a GPU; tests/test_coords_gpu.py then checks what only runs on the device (the kernels'
indexing, launch shapes, fp32 paths, the chain kernels), and a failure there points at a kernel wrapper.  Each test prints its worst error."""
import numpy as np
import pytest
import dojo_amd as d
from oracle import Oracle
import fd_coords as F
from coords_emu_wrap import CoordsEmu
from test_oracle_minimal import JOINT_TYPES

MECHS = [(n, jt) for jt in JOINT_TYPES for n in ("snake", "twister")] + [("quadruped", None)]
H_RICH = 1e-3          # step of the Richardson reference: measured good to 1.4e-10 on these inputs at max |J| up to 81


@pytest.mark.parametrize("name,joint_type", MECHS)
def test_maps_against_the_oracle(name, joint_type):
    """joint_min2max over the bodies root to leaves and joint_max2min, fp64, against the oracle's maps: <= 1e-11 max(1, |ref|) entry by entry"""
    spec = F.joint_type_mechanism(name, joint_type)
    o, e = Oracle(spec), CoordsEmu(spec)
    worst = [0.0, 0.0, 0.0]
    for x in F.edge_inputs(spec):
        z_ref = o.minimal_to_maximal(x)
        x_ref = o.maximal_to_minimal(z_ref)
        ez = np.abs(e.minimal_to_maximal(x) - z_ref) / np.maximum(1.0, np.abs(z_ref))
        ex = np.abs(e.maximal_to_minimal(z_ref) - x_ref) / np.maximum(1.0, np.abs(x_ref))
        worst = [max(worst[0], ez.max()), max(worst[1], ex.max()), max(worst[2], np.abs(x_ref - x).max())]
        assert ez.max() <= 1e-11 and ex.max() <= 1e-11, (ez.max(), ex.max())
    print("coords emu maps %s %s: min2max %.2e max2min %.2e (oracle round trip %.2e)" % (name, joint_type, *worst))


@pytest.mark.parametrize("name,joint_type", MECHS)
def test_jacobians_against_richardson_differences_of_the_oracle(name, joint_type):
    """the Dual<24> evaluations (seeded like seed_body) against (4 D(h/2) - D(h)) / 3 of the oracle's maps, h = 1e-3: <= 5e-9 max(1, max |J_ref|), 35 times
    the reference's own error; a wrong sign, factor or column is >= 1e-2"""
    spec = F.joint_type_mechanism(name, joint_type)
    o, e = Oracle(spec), CoordsEmu(spec)
    worst = [0.0, 0.0]
    for x in F.edge_inputs(spec):
        z = o.minimal_to_maximal(x)
        Jm_ref, JM_ref = F.fd_coordinate_jacobians(o, x, z, H_RICH, richardson=True)
        em = np.abs(e.minimal_to_maximal_jacobian(x) - Jm_ref).max() / max(1.0, np.abs(Jm_ref).max())
        eM = np.abs(e.maximal_to_minimal_jacobian(z) - JM_ref).max() / max(1.0, np.abs(JM_ref).max())
        worst = [max(worst[0], em), max(worst[1], eM)]
        assert em <= 5e-9 and eM <= 5e-9, (em, eM)
    print("coords emu jacobians %s %s: min2max %.2e max2min %.2e" % (name, joint_type, *worst))


def test_richardson_option_leaves_the_default_alone_and_is_sharper():
    """fd_coordinate_jacobians: without the option the result is the plain central difference it always was; with it the error against the Dual<24>
    Jacobian (pinned above) drops by orders of magnitude"""
    spec = F.joint_type_mechanism("snake", "Orbital")
    o, e = Oracle(spec), CoordsEmu(spec)
    x = F.edge_inputs(spec)[9]
    z = o.minimal_to_maximal(x)
    Jm0, JM0 = F.fd_coordinate_jacobians(o, x, z)
    Jm1, JM1 = F._central_differences(o, x, z, 1e-6)
    assert np.array_equal(Jm0, Jm1) and np.array_equal(JM0, JM1)
    JmR, JMR = F.fd_coordinate_jacobians(o, x, z, H_RICH, richardson=True)
    JmH, JMH = F._central_differences(o, x, z, H_RICH)
    J = e.maximal_to_minimal_jacobian(z)
    assert np.abs(JMR - J).max() < 1e-3 * np.abs(JMH - J).max()
    assert np.array_equal(JMR, (4.0 * F._central_differences(o, x, z, 0.5 * H_RICH)[1] - JMH) / 3.0)


def test_edge_inputs_hold_what_they_promise():
    spec = F.joint_type_mechanism("snake", "PlanarAxis")
    X = F.edge_inputs(spec)
    assert len(X) == len(F.EDGE_MAGNITUDES) + 2 and np.array_equal(X, F.edge_inputs(spec))           # seeded
    X65 = F.edge_inputs(spec, 65, seed=3)
    assert len(np.unique(X65, axis=0)) == 65                                                        # every environment a row of its own
    for X_ in (X, X65):
        for r, x in enumerate(X_):
            mag, vel = F.EDGE_ROWS[r % len(F.EDGE_ROWS)]
            o_ = 0
            for j in spec.joints:
                n, nt = j.nu, j.tra.nu
                assert np.abs(x[o_:o_ + nt]).max(initial=0.0) <= 0.3 and np.abs(x[o_ + n:o_ + 2 * n]).max(initial=0.0) <= vel
                if n > nt:
                    assert abs(np.linalg.norm(x[o_ + nt:o_ + n]) - mag) <= 1e-15 * mag
                o_ += 2 * n
    # the magnitudes sit on both sides of both switches of dojo_coords.hpp
    m = np.array(F.EDGE_MAGNITUDES)
    assert (m == 0).any() and ((m > 0) & (m < 1e-6)).sum() >= 2 and ((m > 1e-6) & (m < 4e-6)).sum() >= 2 and ((m > 4e-6) & (m < 1e-4)).sum() >= 2 and (m > np.pi).sum() >= 2


@pytest.mark.parametrize("name,joint_type", [("snake", "PlanarAxis"), ("snake", "Spherical"), ("twister", "Orbital"), ("twister", "PlanarFree"), ("quadruped", None)])
def test_one_joint_map_chained_is_the_oracle_map(name, joint_type):
    """joint_minimal_to_maximal (the helper the fp32-ABI test of the device applies to the parent block the device wrote) reproduces
    oracle.minimal_to_maximal to 1e-10 when it is fed unrounded parents, root to leaves"""
    from dojo_amd.coords import _root_to_leaves
    spec = F.joint_type_mechanism(name, joint_type)
    o = Oracle(spec)
    offs = np.concatenate([[0], np.cumsum([2 * j.nu for j in spec.joints])])
    worst = 0.0
    for x in F.edge_inputs(spec):
        z = np.zeros(13 * spec.Nb)
        for k in _root_to_leaves(spec):
            j = spec.joints[k]
            z[13 * j.child:13 * j.child + 13] = F.joint_minimal_to_maximal(spec, k, None if j.parent < 0 else z[13 * j.parent:13 * j.parent + 13], x[offs[k]:offs[k + 1]])
        worst = max(worst, np.abs(z - o.minimal_to_maximal(x)).max())
    print("one-joint map chained %s %s: %.2e" % (name, joint_type, worst))
    assert worst <= 1e-10


# ---- the chain-kernel test of the GPU tier (tests/test_coords_gpu.py::test_chain_kernels_*): its inputs and its fp64 bound, settled on the CPU ----
@pytest.mark.parametrize("case", F.CHAIN_JOINT_TYPES + ("cartpole",))
def test_chain_inputs_converge_and_reference_noise(case):
    """on every row of the chain test's inputs the oracle's step converges, and jx_ref = JM_ref dz Jm_ref (the oracle's dz) moves by no more than
    CHAIN_NOISE when the Richardson step doubles -- so 50 x that is a bound the reference itself cannot violate"""
    spec = F.chain_mechanism(case)
    o = Oracle(spec, opts=d.SolverOptions(**F.CHAIN_OPTS))
    X, U = F.chain_inputs(spec, o)
    noise = noise_chained = 0.0
    for b in range(len(X)):
        zn, info = o.step(o.minimal_to_maximal(X[b]), U[b])
        assert info["status"] == 0, (case, b)
        for mode in (0, 1):
            dz, _ = o.gradients(mode)
            xp, zp = F.chain_points(spec, o, X[b], zn, mode)
            ref = []
            for h in (H_RICH, 2 * H_RICH):
                Jm, JM = F.fd_coordinate_jacobians(o, xp, zp, h, richardson=True)
                ref.append(JM @ dz @ Jm)
            noise = max(noise, np.abs(ref[0] - ref[1]).max() / max(1.0, np.abs(ref[0]).max()))
            if mode == 0 and b < len(F.CHAIN_ROWS) + 6:          # the literal evaluation's reference (below), one cycle of the rows
                ch = [JM @ dz @ F.fd_chained_minimal_to_maximal_jacobian(spec, xp, zn, h) for h in (H_RICH, 2 * H_RICH)]
                noise_chained = max(noise_chained, np.abs(ch[0] - ch[1]).max() / max(1.0, np.abs(ch[0]).max()))
    print("chain reference noise %s: %.2e (blocks chained at the state after the step: %.2e)" % (case, noise, noise_chained))
    assert noise <= F.CHAIN_NOISE and F.CHAIN_BOUND_F64 == 50 * F.CHAIN_NOISE and F.CHAIN_BOUND_F64 <= 1e-7
    assert noise_chained <= F.CHAIN_NOISE


@pytest.mark.parametrize("name,joint_type", [("snake", "Orbital"), ("snake", "PlanarAxis"), ("twister", "CylindricalFree"), ("cartpole", None)])
def test_chained_blocks_are_the_jacobian_of_the_map_at_consistent_states(name, joint_type):
    """fd_chained_minimal_to_maximal_jacobian (per-joint blocks from differences of the one-joint map, chained root to leaves) at z = minimal_to_maximal(x)
    against the differences of the oracle's whole map: two references that share no code agree within the bound of the Jacobian tests"""
    spec = F.joint_type_mechanism(name, joint_type)
    o = Oracle(spec)
    worst = 0.0
    for x in F.edge_inputs(spec)[[0, 3, 6, 9, 12, 13]]:
        Jm_ref, _ = F.fd_coordinate_jacobians(o, x, o.minimal_to_maximal(x), H_RICH, richardson=True)
        worst = max(worst, np.abs(F.fd_chained_minimal_to_maximal_jacobian(spec, x, o.minimal_to_maximal(x), H_RICH) - Jm_ref).max() / max(1.0, np.abs(Jm_ref).max()))
    print("chained blocks against the whole map %s %s: %.2e" % (name, joint_type, worst))
    assert worst <= 5e-9


def test_literal_evaluation_point_of_the_minimal_gradients():
    """DOJO_GRAD_REFERENCE takes the min -> max Jacobian at the body states after the step, z_next, and the coordinates x_next = maximal_to_minimal(z_next)
    (min2max_jac_kernel reads the parents from its z buffer).  On an Orbital joint (two rotational degrees of freedom) with a rotation and a velocity
    minimal_to_maximal(x_next) is NOT z_next: the joint's coordinates keep two components of the relative angular velocity.  There the chain of blocks is
    no longer the Jacobian of the whole map at x_next, and the device test's reference for this mode has to be the chain at the state (the host
    instantiation of the template agrees with it to the bound of the Jacobian tests, and is far from the Jacobian of the map)."""
    spec = F.chain_mechanism("Orbital")
    o, e = Oracle(spec, opts=d.SolverOptions(**F.CHAIN_OPTS)), CoordsEmu(spec)
    X, U = F.chain_inputs(spec, o)
    b = 59                                          # a synthetic row: joint angles of 0.1 .. 0.9, velocities of 0.1 .. 1.1
    zn, info = o.step(o.minimal_to_maximal(X[b]), U[b])
    assert info["status"] == 0
    xn = o.maximal_to_minimal(zn)
    gap = (o.minimal_to_maximal(xn) - zn).reshape(spec.Nb, 13)
    assert np.abs(gap[:, [0, 1, 2, 6, 7, 8, 9]]).max() < 1e-9 and np.abs(gap[:, 10:13]).max() > 0.1      # poses round-trip, angular velocities do not
    J_state = e.minimal_to_maximal_jacobian(xn, zn)
    ref_state = F.fd_chained_minimal_to_maximal_jacobian(spec, xn, zn, H_RICH)
    ref_map, _ = F.fd_coordinate_jacobians(o, xn, zn, H_RICH, richardson=True)
    err_state, err_map = np.abs(J_state - ref_state).max(), np.abs(J_state - ref_map).max()
    print("literal evaluation point, Orbital: round-trip gap %.2e; template at the state against the chained blocks %.2e, against the map's Jacobian %.2e"
          % (np.abs(gap).max(), err_state, err_map))
    assert err_state <= 5e-9 * max(1.0, np.abs(ref_state).max()) and err_map > 1e-2
