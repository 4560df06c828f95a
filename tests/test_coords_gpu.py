"""The coordinate kernels of dojo.jl_amd/csrc/dojo_coord_kernels.hpp (min2max_kernel, max2min_kernel, min2max_jac_kernel, max2min_jac_kernel, chain_mid_kernel,
chain_out_kernel, next_state_kernel) and observation_jacobian_kernel on the device, against the C++ oracle: every joint prototype, rotations at 0, on either
side of the series switches of dojo_coords.hpp and beyond pi (tests/fd_coords.py: edge_inputs), fp64 and fp32 handles, batches that end inside a block
and environments that straddle one.  Every environment of a batch has an input row of its own and every environment is compared unless a test says
otherwise.  The templates themselves are pinned on the host by tests/test_coords_emu.py, so a failure here points at a kernel's indexing or launch.
Each test prints its worst error."""
import numpy as np
import pytest
import dojo_amd as d
from dojo_amd import api, coords
from dojo_amd.quat import next_orientation
from oracle import Oracle
import fd_coords as F
from test_oracle_minimal import JOINT_TYPES

pytestmark = pytest.mark.gpu

MECHS = [(n, jt) for jt in JOINT_TYPES for n in ("snake", "twister")]
F32_TYPES = ["Revolute", "Prismatic", "PlanarAxis", "Orbital", "Spherical", "PlanarFree"]
H_RICH = 1e-3
ULP32 = 2.0 ** -23
_cache = {}


def _case(name, joint_type, B, seed=11):
    """(spec, oracle, X [B, 2nu] edge inputs, Z = oracle.minimal_to_maximal(X), oracle.maximal_to_minimal(Z)), computed once per case"""
    key = (name, joint_type, B, seed)
    if key not in _cache:
        spec = F.joint_type_mechanism(name, joint_type)
        o = Oracle(spec)
        X = F.edge_inputs(spec, B, seed=seed)
        Z = np.stack([o.minimal_to_maximal(x) for x in X])
        Xr = np.stack([o.maximal_to_minimal(z) for z in Z])
        for a in (X, Z, Xr):
            a.setflags(write=False)
        _cache[key] = (spec, o, X, Z, Xr)
    return _cache[key]


def _maps_fp64(name, joint_type, B):
    """both maps of an fp64 handle at every environment -> per-environment errors (min2max, max2min, round trip)"""
    spec, o, X, Z, Xr = _case(name, joint_type, B)
    gm = api.BatchedMechanism(spec, B, dtype="f64")
    Zd = gm.minimal_to_maximal(X); Xd = gm.maximal_to_minimal(Z); Xrt = gm.maximal_to_minimal(Zd)
    gm.close()
    assert np.isfinite(Zd).all() and np.isfinite(Xd).all() and np.isfinite(Xrt).all()
    return np.abs(Zd - Z).max(axis=1), np.abs(Xd - Xr).max(axis=1), np.abs(Xrt - X).max(axis=1)


# ---- a. maps, fp64, every joint type ----
@pytest.mark.parametrize("name,joint_type", MECHS + [("quadruped", None)])
def test_maps_fp64_every_joint_type(name, joint_type):
    """minimal_to_maximal / maximal_to_minimal of an fp64 handle against the oracle at <= 1e-10 (the bound of test_minimal_maximal_maps) and the round
    trip max2min(min2max(X)) against X at 1e-8, B = 65, all environments.  The quadruped case has its floating base's rotation (and every leg joint)
    at the edge magnitudes.  Observed on an MI355X over the 31 cases: min2max 2.2e-13, max2min 1.0e-13, round trip 1.2e-13."""
    ez, ex, ert = _maps_fp64(name, joint_type, 65)
    print("coords gpu maps fp64 %s %s: min2max %.2e max2min %.2e round trip %.2e" % (name, joint_type, ez.max(), ex.max(), ert.max()))
    assert ez.max() <= 1e-10 and ex.max() <= 1e-10, (ez.argmax(), ez.max(), ex.argmax(), ex.max())
    assert ert.max() <= 1e-8, (ert.argmax(), ert.max())


# ---- b. shapes ----
def _straddlers(B, Nb, T=256):
    """environments whose Nb threads of max2min_kernel (T threads per block, thread = env * Nb + joint) lie in two blocks"""
    return [e for e in range(B) if (e * Nb) // T != (e * Nb + Nb - 1) // T]


@pytest.mark.parametrize("joint_type", ["PlanarAxis", "Spherical"])
@pytest.mark.parametrize("B", [1, 63, 65, 257])
def test_maps_at_ragged_batches(joint_type, B):
    """min2max_kernel runs 64 threads per block, one per environment; max2min_kernel 256 threads over B x Nb with env = tid / Nb.  Batches of one, one
    short of a block, one over a block (the last min2max block holds ONE environment) and 257 (Nb = 3: the environments 85 and 170 have their joints
    in two max2min blocks; the last block of either kernel is partial): every environment at 1e-10, the first, the last and the straddlers by name"""
    Nb = 3
    ez, ex, ert = _maps_fp64("snake", joint_type, B)
    named = {0, B - 1}
    if B == 65:
        assert B % 64 == 1
    if B == 257:
        assert _straddlers(B, Nb) == [85, 170] and (B * Nb) % 256 != 0 and B % 64 != 0
        named |= {84, 85, 86, 169, 170, 171}
    assert len(ez) == len(ex) == B
    for e in sorted(named):
        assert ez[e] <= 1e-10 and ex[e] <= 1e-10 and ert[e] <= 1e-8, (e, ez[e], ex[e], ert[e])
    print("coords gpu shapes %s B=%d: min2max %.2e max2min %.2e round trip %.2e" % (joint_type, B, ez.max(), ex.max(), ert.max()))
    assert ez.max() <= 1e-10 and ex.max() <= 1e-10 and ert.max() <= 1e-8, (ez.argmax(), ez.max(), ex.argmax(), ex.max())


# ---- c. fp32 ABI ----
def _differing(got, ref):
    return int((np.asarray(got) != np.asarray(ref)).sum())


def _ulp_excess(got, ref):
    """largest (|got - ref| - bound) over the entries, bound = 2^-23 |ref| + 1e-10: both sides compute in fp64 from the same rounded inputs and round the
    result once, so they differ by a flipped rounding (one ulp) at the most"""
    got = np.asarray(got, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    return (np.abs(got - ref) - (ULP32 * np.abs(ref) + 1e-10)).max()


@pytest.mark.parametrize("name", ["snake", "twister"])
@pytest.mark.parametrize("joint_type", F32_TYPES)
def test_maps_fp32_abi(name, joint_type):
    """an fp32 handle.  max2min: against float32(oracle(fp32_abi_state(Z32))).  min2max: the kernel reads each parent back from the fp32 buffer it has just
    written (load_body renormalises it), so it is checked joint by joint -- the child block the device wrote against float32 of the one-joint map
    (fd_coords.joint_minimal_to_maximal, pinned in tests/test_coords_emu.py) of fp32_abi_state of the parent block THE DEVICE wrote and the rounded
    joint coordinates.  Entry-wise bound 2^-23 |ref| + 1e-10."""
    B = 65
    spec, o, X, Z, _ = _case(name, joint_type, B)
    X32 = X.astype(np.float32); Z32 = Z.astype(np.float32)
    gm = api.BatchedMechanism(spec, B, dtype="f32")
    Xd = gm.maximal_to_minimal(Z32); Zd = gm.minimal_to_maximal(X32)
    gm.close()
    assert Xd.dtype == np.float32 and Zd.dtype == np.float32 and np.isfinite(Xd).all() and np.isfinite(Zd).all()
    Zs = d.fp32_abi_state(Z32)
    Xref = np.stack([o.maximal_to_minimal(Zs[b]) for b in range(B)]).astype(np.float32)
    ex, nx_ = _ulp_excess(Xd, Xref), _differing(Xd, Xref)
    offs = np.concatenate([[0], np.cumsum([2 * j.nu for j in spec.joints])])
    Zp = d.fp32_abi_state(Zd)                                   # the states the device's blocks stand for when they are read back as parents
    ez, nz_ = -np.inf, 0
    for b in range(B):
        for k, j in enumerate(spec.joints):
            ref = F.joint_minimal_to_maximal(spec, k, None if j.parent < 0 else Zp[b, 13 * j.parent:13 * j.parent + 13], X32[b, offs[k]:offs[k + 1]].astype(np.float64))
            ez = max(ez, _ulp_excess(Zd[b, 13 * j.child:13 * j.child + 13], ref.astype(np.float32)))
            nz_ += _differing(Zd[b, 13 * j.child:13 * j.child + 13], ref.astype(np.float32))
    print("coords gpu maps fp32 %s %s: largest |error| - (2^-23 |ref| + 1e-10): max2min %.2e (%d of %d entries not the reference's bits) min2max %.2e (%d of %d)"
          % (name, joint_type, ex, nx_, Xd.size, ez, nz_, Zd.size))
    assert ex <= 0.0 and ez <= 0.0, (ex, ez)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_next_state(dtype):
    """dojo_next_state (next_state_kernel: one thread per (environment, body), 256 per block, 257 x 3 threads) against x + dt v and
    quat.next_orientation; fp64 at 1e-12, fp32 at one ulp of the rounded reference"""
    B = 257
    spec, o, X, Z, _ = _case("snake", "Spherical", B)
    gm = api.BatchedMechanism(spec, B, dtype=dtype)
    Zin = Z.astype(gm.np_dtype)
    Zo = gm.next_state(Zin)
    gm.close()
    Zs = d.fp32_abi_state(Zin) if dtype == "f32" else Z
    ref = Zs.copy().reshape(B, spec.Nb, 13)
    dt = spec.timestep
    for b in range(B):
        for k in range(spec.Nb):
            ref[b, k, 0:3] += dt * ref[b, k, 3:6]
            ref[b, k, 6:10] = next_orientation(ref[b, k, 6:10], ref[b, k, 10:13], dt)
    ref = ref.reshape(B, -1)
    assert np.isfinite(Zo).all()
    if dtype == "f64":
        err = np.abs(Zo - ref).max(axis=1)
        print("coords gpu next_state f64: %.2e" % err.max())
        assert err.max() <= 1e-12, (err.argmax(), err.max())
    else:
        ex = _ulp_excess(Zo, ref.astype(np.float32))
        print("coords gpu next_state f32: largest |error| - (2^-23 |ref| + 1e-10) = %.2e" % ex)
        assert ex <= 0.0


# ---- d. the max2min Jacobian alone ----
def _observation_jacobian_errors(name, joint_type, B, dtype, envs):
    spec, o, X, Z, _ = _case(name, joint_type, B)
    gm = api.BatchedMechanism(spec, B, dtype=dtype)
    Zin = Z.astype(gm.np_dtype)
    Mc = gm.observation_jacobian(Zin)
    gm.close()
    assert np.isfinite(Mc).all()
    r = 0
    for j in spec.joints:                   # a joint on the origin has no parent: its parent columns are written as exact zeros
        if j.parent < 0:
            assert not Mc[:, r:r + 2 * j.nu, 0:12].any()
        r += 2 * j.nu
    J = coords.dense_observation_jacobian(spec, Mc)
    Zs = d.fp32_abi_state(Zin) if dtype == "f32" else Z
    err = {}
    for b in envs:
        _, JM = F.fd_coordinate_jacobians(o, o.maximal_to_minimal(Zs[b]), Zs[b], H_RICH, richardson=True)
        err[b] = np.abs(J[b] - JM).max() / max(1.0, np.abs(JM).max())
    return err


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,joint_type", MECHS)
def test_observation_jacobian_every_joint_type(name, joint_type, dtype):
    """gm.observation_jacobian (observation_jacobian_kernel: the Dual<24> evaluation max2min_jac_kernel is made of), densified, against the Richardson
    reference of the oracle's map at Z (fp64 handle) or at fp32_abi_state(Z) (fp32 handle: the kernel computes in fp64 from the state the buffer stands
    for): <= 5e-9 max(1, max |J_ref|) at every environment of B = 65.  The existing test allows 1e-6 on three mechanisms.
    Observed on an MI355X over the 30 mechanisms: 6.4e-11 (fp64 handle), 7.8e-11 (fp32 handle)."""
    err = _observation_jacobian_errors(name, joint_type, 65, dtype, range(65))
    worst = max(err, key=err.get)
    print("coords gpu observation jacobian %s %s %s: %.2e (environment %d)" % (dtype, name, joint_type, err[worst], worst))
    assert err[worst] <= 5e-9, (worst, err[worst])


@pytest.mark.parametrize("joint_type", ["PlanarAxis", "Spherical"])
def test_observation_jacobian_across_blocks(joint_type):
    """B = 257, Nb = 3: 128 threads per block over B x Nb -- environments around the block boundaries of either coordinate launch shape and the last one.
    Observed on an MI355X: <= 4.2e-11 at each of them."""
    envs = [0, 84, 85, 86, 170, 171, 256]
    err = _observation_jacobian_errors("snake", joint_type, 257, "f64", envs)
    print("coords gpu observation jacobian B=257 %s: %s" % (joint_type, " ".join("%d:%.2e" % (b, err[b]) for b in envs)))
    assert sorted(err) == envs
    for b in envs:
        assert err[b] <= 5e-9, (b, err[b])


# ---- e. the min2max Jacobian and the chain kernels, isolated from the IFT ----
def _chain_errors(case, dtype, mode):
    """jx, ju of gm.minimal_gradients against JM_ref(zp) dz Jm_ref(xp), JM_ref(zp) du with the DEVICE's own dz, du (and its own next state), so that solver
    and IFT differences cancel and what is left is min2max_jac_kernel, max2min_jac_kernel, chain_mid_kernel and chain_out_kernel"""
    B = F.CHAIN_BATCH
    spec = F.chain_mechanism(case)
    opts = d.SolverOptions(**F.CHAIN_OPTS)
    o = Oracle(spec, opts=opts)
    X, U = F.chain_inputs(spec, o, B)
    gm = api.BatchedMechanism(spec, B, dtype=dtype, opts=opts)
    gm.set_gradient_mode(mode)
    Xin = X.astype(gm.np_dtype); Uin = U.astype(gm.np_dtype)
    zn, st, it = gm.step(gm.minimal_to_maximal(Xin), Uin, with_gradient=True)
    dz, du = gm.gradients()
    xn, st2, it2, jx, ju = gm.minimal_gradients(Xin, Uin)
    gm.close()
    assert np.array_equal(st, st2) and np.array_equal(it, it2)          # the same solve (test_step_minimal_coordinates)
    ok = np.flatnonzero(st == 0)
    assert len(ok) >= 0.9 * B, (len(ok), B)
    ex, eu, emap = {}, {}, {}

    def err(got, ref):              # fp64: relative to the largest entry; fp32: entry-wise 1e-4 max(1, |ref|)
        return np.abs(got - ref).max() / max(1.0, np.abs(ref).max()) if dtype == "f64" else (np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()
    for b in ok:
        # the points the buffers stand for: an fp32 handle reads x, x_next and z_next back from fp32
        x_in, z_out = (Xin[b].astype(np.float64), d.fp32_abi_state(zn[b:b + 1])[0]) if dtype == "f32" else (X[b], zn[b])
        xp, zp = F.chain_points(spec, o, x_in, z_out, mode)
        Jm, JM = F.fd_coordinate_jacobians(o, xp, zp, H_RICH, richardson=True)
        D = dz[b].astype(np.float64)
        assert np.isfinite(jx[b]).all() and np.isfinite(ju[b]).all()
        if mode == 0:
            # the literal evaluation takes the blocks of the min -> max Jacobian at the body states after the step (include/dojo_hip.h); that is the Jacobian
            # of the map x -> z, Jm above, only where minimal_to_maximal(maximal_to_minimal(z_next)) = z_next (fd_chained_minimal_to_maximal_jacobian)
            emap[b] = err(jx[b], JM @ D @ Jm)
            Jm = F.fd_chained_minimal_to_maximal_jacobian(spec, xn[b].astype(np.float64) if dtype == "f32" else xp, z_out, H_RICH)
        ex[b] = err(jx[b], JM @ D @ Jm)
        eu[b] = err(ju[b], JM @ du[b].astype(np.float64))
    if emap:
        bm = max(emap, key=emap.get)
        print("coords gpu chain %s %s mode 0: jx against JM dz Jm_map(x_next), the Jacobian of the whole map: %.2e (environment %d)" % (dtype, case, emap[bm], bm))
    return ex, eu, B - len(ok)


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("case", F.CHAIN_JOINT_TYPES + ("cartpole",))
def test_chain_kernels_fp64(case, mode):
    """<= F.CHAIN_BOUND_F64 max(1, max |ref|) = 3.0e-8: 50 times the reference's own noise, 6.0e-10, measured on these inputs with the oracle's dz by
    tests/test_coords_emu.py::test_chain_inputs_converge_and_reference_noise (fd_coords.CHAIN_NOISE).  test_minimal_gradients allows 2e-5.
    mode 0 (DOJO_GRAD_REFERENCE) runs advance = 1 and xj = x_next, and min2max_jac_kernel reads the parents from the state after the step: the reference's
    min -> max Jacobian for that mode is the chain of per-joint blocks AT THAT STATE (fd_coords.fd_chained_minimal_to_maximal_jacobian; the same as the
    Jacobian of the whole map wherever minimal_to_maximal(x_next) = z_next, tests/test_coords_emu.py).  Against JM dz Jm_map(x_next) with the whole map's
    Jacobian, which _check_minimal_gradients uses, the device is at 1.7e-1 on the Orbital snake (environment 59: the joint's two coordinates cannot hold the
    relative angular velocity of z_next, the round trip misses it by 0.24) and at 2.2e-8 on the Revolute one (joints closed to the solver's tolerance,
    velocities of 20); that figure is printed, not asserted.
    Observed on an MI355X over the six cases: mode 1 jx 3.0e-10, ju 7.0e-11; mode 0 jx 3.4e-10, ju 7.4e-11; every environment converged."""
    ex, eu, left_out = _chain_errors(case, "f64", mode)
    bx, bu = max(ex, key=ex.get), max(eu, key=eu.get)
    print("coords gpu chain f64 %s mode %d: jx %.2e (environment %d) ju %.2e (environment %d), %d not converged" % (case, mode, ex[bx], bx, eu[bu], bu, left_out))
    assert ex[bx] <= F.CHAIN_BOUND_F64 and eu[bu] <= F.CHAIN_BOUND_F64, (bx, ex[bx], bu, eu[bu])


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("case", F.CHAIN_JOINT_TYPES + ("cartpole",))
def test_chain_kernels_fp32(case, mode):
    """an fp32 handle: 1e-4 max(1, |ref|) entry by entry, the project's fp32 Jacobian bound (test_gradients_of_a_forest_on_the_device), the reference at
    the points the fp32 buffers stand for (mode 0: the blocks chained at fp32_abi_state(z_next) and the x_next the device returned, as in the fp64 test).
    Observed on an MI355X: mode 1 jx 1.3e-5 (the kernel reads the parents from the fp32 state minimal_to_maximal wrote, 1e-7 from the map of the
    rounded x, and the velocity rows carry 1 / dt), ju 5.8e-8; mode 0 jx 6.0e-8, ju 5.8e-8."""
    ex, eu, left_out = _chain_errors(case, "f32", mode)
    bx, bu = max(ex, key=ex.get), max(eu, key=eu.get)
    print("coords gpu chain f32 %s mode %d: jx %.2e (environment %d) ju %.2e (environment %d), %d not converged" % (case, mode, ex[bx], bx, eu[bu], bu, left_out))
    assert ex[bx] <= 1e-4 and eu[bu] <= 1e-4, (bx, ex[bx], bu, eu[bu])
