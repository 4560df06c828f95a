"""Finite-difference coordinate Jacobians of the ORACLE's minimal <-> maximal maps (test helper, shared by the CPU and GPU tiers).

Restates minimal_to_maximal_jacobian(x) [12Nb x 2nu] (src/gradients/state.jl:128-179) and maximal_to_minimal_jacobian(z)
[2nu x 12Nb] (src/gradients/state.jl:1-56) by central differences of the oracle's maps (pinned by test/minimal.jl restated,
tests/test_oracle_minimal.py), with the attitude convention dq = q (x) (sqrt(1-|phi|^2), phi) of the reference's attitude Jacobians.

Also the inputs of the coordinate-kernel tests (tests/test_coords_emu.py, tests/test_coords_gpu.py): minimal states whose joint rotations sit on
either side of the series switches of dojo_coords.hpp (aa2qS at |r| = 1e-6, rotvecS at a rotation of about 4e-6), at 0 and beyond pi, and the
one-joint map the fp32-ABI test applies to the parent block the device wrote.
"""
import numpy as np
from dojo_amd.quat import qmul, qconj


def _central_differences(o, xp, zp, h):
    Nb, nm = o.Nb, 2 * o.nu

    def reduce(zd, z0):                       # maximal difference quotient -> [x v phi w] per body
        out = np.zeros(12 * Nb)
        for b in range(Nb):
            out[12 * b:12 * b + 6] = zd[13 * b:13 * b + 6]
            out[12 * b + 6:12 * b + 9] = qmul(qconj(z0[13 * b + 6:13 * b + 10]), zd[13 * b + 6:13 * b + 10])[1:]
            out[12 * b + 9:12 * b + 12] = zd[13 * b + 10:13 * b + 13]
        return out
    z0 = o.minimal_to_maximal(xp)
    Jm = np.zeros((12 * Nb, nm))
    for j in range(nm):
        e = np.zeros(nm); e[j] = h
        Jm[:, j] = reduce((o.minimal_to_maximal(xp + e) - o.minimal_to_maximal(xp - e)) / (2 * h), z0)
    JM = np.zeros((nm, 12 * Nb))
    for b in range(Nb):
        for i in range(12):
            zs = []
            for sgn in (1.0, -1.0):
                z = zp.copy()
                if i < 6: z[13 * b + i] += sgn * h
                elif i < 9:
                    ph = np.zeros(3); ph[i - 6] = sgn * h
                    z[13 * b + 6:13 * b + 10] = qmul(zp[13 * b + 6:13 * b + 10], np.concatenate([[np.sqrt(1 - h * h)], ph]))
                else: z[13 * b + 10 + (i - 9)] += sgn * h
                zs.append(o.maximal_to_minimal(z))
            JM[:, 12 * b + i] = (zs[0] - zs[1]) / (2 * h)
    return Jm, JM


def fd_coordinate_jacobians(o, xp, zp, h=1e-6, richardson=False):
    """o: oracle.Oracle of the mechanism; xp: minimal state the min->max Jacobian is taken at; zp: maximal state of the max->min one.
    richardson: (4 D(h/2) - D(h)) / 3 of the central differences D -- the h^2 term of the truncation error cancels, so a step of 1e-3
    (rounding error 1e-16 / 1e-3) leaves about 1e-10 where h = 1e-6 leaves 5e-8"""
    if not richardson:
        return _central_differences(o, xp, zp, h)
    Jm1, JM1 = _central_differences(o, xp, zp, h)
    Jm2, JM2 = _central_differences(o, xp, zp, 0.5 * h)
    return (4.0 * Jm2 - Jm1) / 3.0, (4.0 * JM2 - JM1) / 3.0


# rotation magnitudes of the edge inputs: 0 (both series), either side of aa2qS's switch (|r| = 1e-6) and of rotvecS's (|m| = 1e-6: a rotation
# of 4e-6), small and generic angles, and three beyond / near pi (q0 <= 0, where 1 / (1 + q0) of the rotation vector grows)
EDGE_MAGNITUDES = (0.0, 1e-9, 5e-7, 0.999e-6, 1.001e-6, 3.9e-6, 4.1e-6, 1e-5, 1e-3, 1.0, 3.0, 1.2 * np.pi, 1.5 * np.pi)
# (rotation magnitude, bound of the minimal velocities) of the standard rows: every magnitude with velocities within +-1, two rows within +-20
EDGE_ROWS = tuple((m, 1.0) for m in EDGE_MAGNITUDES) + ((1.0, 20.0), (3.9e-6, 20.0))


def edge_minimal_states(spec, magnitudes, seed=0, velocity=1.0):
    """one minimal state per entry of `magnitudes`: every joint's rotational coordinates are a random direction (of the joint's nu_r coordinates)
    scaled to the magnitude, its translational coordinates uniform in +-0.3, its minimal velocities uniform in +-velocity (a number, or one per row)"""
    rng = np.random.default_rng(seed)
    vel = np.broadcast_to(np.asarray(velocity, dtype=float), (len(magnitudes),))
    X = np.zeros((len(magnitudes), 2 * spec.nu))
    for r, mag in enumerate(magnitudes):
        o = 0
        for j in spec.joints:
            n, nt = j.nu, j.tra.nu
            X[r, o:o + nt] = rng.uniform(-0.3, 0.3, nt)
            if n > nt:
                d = rng.standard_normal(n - nt)
                X[r, o + nt:o + n] = mag * d / np.linalg.norm(d)
            X[r, o + n:o + 2 * n] = rng.uniform(-vel[r], vel[r], n)
            o += 2 * n
    return X


def edge_inputs(spec, n=None, seed=0, rows=EDGE_ROWS):
    """n minimal states (default: one per entry of `rows`) that cycle through `rows`, every one with directions and values of its own"""
    n = len(rows) if n is None else int(n)
    pick = [rows[i % len(rows)] for i in range(n)]
    return edge_minimal_states(spec, [m for m, _ in pick], seed=seed, velocity=[v for _, v in pick])


def joint_type_mechanism(name, joint_type, contact=True):
    """the mechanisms of the coordinate-kernel tests: "snake" (three bodies, every joint with a random orientation offset, as in test/minimal.jl:65-106)
    or "twister" (four bodies, the joint axis cycling) with `joint_type` between the bodies; "quadruped" (floating base + revolute legs) and "cartpole" as they are"""
    import dojo_amd as d
    if name == "snake":
        spec = d.get_mechanism("snake", num_bodies=3, joint_type=joint_type, contact=contact)
        rng = np.random.default_rng(100)
        for j in spec.joints:
            q = rng.standard_normal(4); j.orientation_offset = q / np.linalg.norm(q)
        return spec
    if name == "twister":
        return d.get_mechanism("twister", num_bodies=4, joint_type=joint_type, contact=contact)
    return d.get_mechanism(name)


# ---- inputs of the chain-kernel tests (jx = JM dz Jm with the step's own dz): shared by the CPU tier, which measures the reference's noise on them and
#      checks that the oracle converges on every row, and the GPU tier ----
CHAIN_JOINT_TYPES = ("Revolute", "PlanarAxis", "Orbital", "Spherical", "CylindricalFree")
CHAIN_BATCH = 65
CHAIN_ROWS = tuple(r for r in EDGE_ROWS if r[0] <= 1e-3)
CHAIN_OPTS = dict(rtol=1e-8, btol=1e-8)
# the reference's noise on these inputs: the largest difference of jx_ref = JM_ref dz Jm_ref (the oracle's dz) between Richardson references of h = 1e-3
# and h = 2e-3, relative to max(1, max |jx_ref|), over all cases, both gradient modes and all rows (tests/test_coords_emu.py measures it again and
# fails if it grows); the fp64 bound of the device test is 50 times that.  Measured: Revolute 5.62e-10, PlanarAxis 2.78e-10, Orbital 2.71e-10,
# Spherical 5.96e-10, CylindricalFree 3.69e-10, cartpole 6.79e-11 -- the largest, rounded up to two digits:
CHAIN_NOISE = 6.0e-10
CHAIN_BOUND_F64 = 50 * CHAIN_NOISE


def chain_mechanism(case):
    """case: one of CHAIN_JOINT_TYPES (a three-body snake without contacts: the step's Jacobian is smooth, so the test sees the coordinate kernels) or "cartpole" """
    return joint_type_mechanism("cartpole", None) if case == "cartpole" else joint_type_mechanism("snake", case, contact=False)


def chain_inputs(spec, oracle, B=CHAIN_BATCH):
    """X [B, 2nu], U [B, nu]: the edge rows of magnitude <= 1e-3 and six rows of the synthetic inputs, cycled, every environment with values of its own"""
    import dojo_amd as d
    ne = len(CHAIN_ROWS)
    Zs, U = d.synthetic_inputs(spec, B)
    Xe = edge_inputs(spec, B, seed=7, rows=CHAIN_ROWS)
    X = np.stack([Xe[b] if b % (ne + 6) < ne else oracle.maximal_to_minimal(Zs[b]) for b in range(B)])     # of every ne + 6 environments: ne edge rows, six synthetic ones
    return X, U


def chain_points(spec, oracle, x, zn, mode):
    """where get_minimal_gradients! evaluates its coordinate Jacobians (tests/test_gpu_parity.py::_check_minimal_gradients): (xp of the min -> max one,
    zp of the max -> min one) from the step's input x and output zn; mode 0 is the reference's literal choice (the new state, advanced once more)"""
    from dojo_amd.quat import next_orientation
    if mode == 1:
        return x, zn
    dt = spec.timestep
    zp = zn.copy()
    for k in range(spec.Nb):
        zp[13 * k:13 * k + 3] = zn[13 * k:13 * k + 3] + dt * zn[13 * k + 3:13 * k + 6]
        zp[13 * k + 6:13 * k + 10] = next_orientation(zn[13 * k + 6:13 * k + 10], zn[13 * k + 10:13 * k + 13], dt)
    return oracle.maximal_to_minimal(zn), zp


def fd_chained_minimal_to_maximal_jacobian(spec, x, z, h=1e-3):
    """minimal_to_maximal_jacobian [12Nb x 2nu] the way src/gradients/state.jl:136-181 builds it: per joint the partials of the child's state w.r.t. the
    parent's tangent coordinates [x; v; phi; omega] and w.r.t. the joint's own coordinates, taken at the PARENT STATE z holds and the joint coordinates x
    holds, chained root to leaves (J[child] = P_parent J[parent] + P_joint).  The partials are Richardson-extrapolated central differences of the one-joint
    map below (pinned against the oracle by tests/test_coords_emu.py).  Where z = minimal_to_maximal(x) this is the Jacobian of the map x -> z, i.e.
    fd_coordinate_jacobians' first result; get_minimal_gradients! in its literal evaluation (DOJO_GRAD_REFERENCE) takes it at z = the state after the
    step and x = maximal_to_minimal(z), and minimal_to_maximal(maximal_to_minimal(z)) is z only up to what the minimal coordinates can hold: a joint with
    two rotational degrees of freedom keeps two components of its relative angular velocity, a solved step closes its joints to the solver's tolerance."""
    from dojo_amd.coords import _root_to_leaves
    x = np.asarray(x, dtype=float); z = np.asarray(z, dtype=float)
    nm = 2 * spec.nu
    offs = np.concatenate([[0], np.cumsum([2 * j.nu for j in spec.joints])])
    J = np.zeros((12 * spec.Nb, nm))

    def partials(k, parent, xm, h_):
        n2 = len(xm)
        q0 = joint_minimal_to_maximal(spec, k, parent, xm)[6:10]

        def reduce(cd):
            return np.concatenate([cd[0:6], qmul(qconj(q0), cd[6:10])[1:], cd[10:13]])
        P = np.zeros((12, 12 + n2))
        for i in range(12 if parent is not None else 0):
            cs = []
            for sgn in (1.0, -1.0):
                p = parent.copy()
                if i < 6: p[i] += sgn * h_
                elif i < 9:
                    ph = np.zeros(3); ph[i - 6] = sgn * h_
                    p[6:10] = qmul(parent[6:10], np.concatenate([[np.sqrt(1 - h_ * h_)], ph]))
                else: p[10 + (i - 9)] += sgn * h_
                cs.append(joint_minimal_to_maximal(spec, k, p, xm))
            P[:, i] = reduce((cs[0] - cs[1]) / (2 * h_))
        for i in range(n2):
            e = np.zeros(n2); e[i] = h_
            P[:, 12 + i] = reduce((joint_minimal_to_maximal(spec, k, parent, xm + e) - joint_minimal_to_maximal(spec, k, parent, xm - e)) / (2 * h_))
        return P
    for k in _root_to_leaves(spec):
        j = spec.joints[k]
        parent = None if j.parent < 0 else z[13 * j.parent:13 * j.parent + 13]
        xm = x[offs[k]:offs[k + 1]]
        P = (4.0 * partials(k, parent, xm, 0.5 * h) - partials(k, parent, xm, h)) / 3.0
        rows = slice(12 * j.child, 12 * j.child + 12)
        if parent is not None:
            J[rows] = P[:, :12] @ J[12 * j.parent:12 * j.parent + 12]
        J[rows, offs[k]:offs[k + 1]] += P[:, 12:]
    return J


def joint_minimal_to_maximal(spec, k, parent, xm):
    """the loop body of dojo_amd.coords.minimal_to_maximal for joint k alone: the 13 numbers of its child body from those of its parent body
    (None: the origin) and the joint's minimal coordinates xm = [dx; dtheta; dv; domega]"""
    from dojo_amd.quat import vrot, qinv, axis_angle_to_quaternion, next_orientation, angular_velocity
    j, dt = spec.joints[k], spec.timestep
    nu, nt = j.nu, j.tra.nu
    xm = np.asarray(xm, dtype=float)
    dx, dth, dv, dw = xm[:nt], xm[nt:nu], xm[nu:nu + nt], xm[nu + nt:]
    if parent is None:
        xa, va, qa, wa = np.zeros(3), np.zeros(3), np.array([1.0, 0, 0, 0]), np.zeros(3)
    else:
        p = np.asarray(parent, dtype=float)
        xa, va, qa, wa = p[0:3], p[3:6], p[6:10], p[10:13]
    _, At = j.tra.masks(); _, Ar = j.rot.masks()
    pa, pb, qoff = j.vertex_parent, j.vertex_child, j.orientation_offset
    dq = axis_angle_to_quaternion(Ar.T @ dth) if Ar.shape[0] else np.array([1.0, 0, 0, 0])
    qb = qmul(qmul(qa, qoff), dq)
    xb = xa + vrot(pa + (At.T @ dx if At.shape[0] else 0.0), qa) - vrot(pb, qb)
    xa1 = xa - va * dt
    qa1 = next_orientation(qa, -wa, dt)
    dx1 = dx - dv * dt
    dq1 = qmul(dq, qinv(axis_angle_to_quaternion(Ar.T @ (dw * dt)))) if Ar.shape[0] else dq
    qb1 = qmul(qmul(qa1, qoff), dq1)
    xb1 = xa1 + vrot(pa + (At.T @ dx1 if At.shape[0] else 0.0), qa1) - vrot(pb, qb1)
    return np.concatenate([xb, (xb - xb1) / dt, qb, angular_velocity(qb1, qb, dt)])
