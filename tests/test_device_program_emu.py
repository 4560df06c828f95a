"""CPU tier: the shipped device source (dojo.jl_amd/csrc/dojo_entries.hpp + dojo_device.hpp) run under the
thread-based SIMT emulator (tests/emu) against the oracle.  Small cases only (the emulator pays
two barriers per wave shuffle); the real parity tests are the -m gpu ones."""
import os
import sys
import numpy as np
import pytest
import dojo_amd as d
from oracle import Oracle
from emu_wrap import emu_step

TIGHT = d.SolverOptions(rtol=1e-8, btol=1e-8)


# quad = True: four lanes per supernode (the mapping the product uses up to 32 bodies); False: one lane per supernode (> 32 bodies)
@pytest.mark.parametrize("cfg,steps,quad", [(1, 3, True), (2, 3, True), (3, 3, True), (4, 2, True), (5, 2, True), (2, 2, False), (3, 1, False)])
def test_forward_matches_oracle(cfg, steps, quad):
    spec = d.baseline_config(cfg)
    o = Oracle(spec, opts=TIGHT)
    Z, U = d.synthetic_inputs(spec, 1)
    z, u = Z[0], U[0]
    for _ in range(steps):
        zo, info = o.step(z, u)
        r = emu_step(spec, z, u, opts=TIGHT, quad=quad)
        assert r["status"][0] == info["status"] == 0
        assert np.abs(r["z_next"][0] - zo).max() < 1e-7
        sol = o.get_solution()
        nj = spec.n_joint_impulses
        assert np.abs(r["vel"][0] - sol[nj:nj + 6 * spec.Nb]).max() < 1e-7
        z = zo


def test_block_in_contact_two_envs_per_wave():
    # two environments share one emulated wave: exercises the per-environment masks / reductions
    spec = d.baseline_config(2)
    o = Oracle(spec, opts=TIGHT)
    z0 = d.initialize(spec, position=[0, 0, 0.02], velocity=[1.0, 0.5, -1.0], angular_velocity=[0.3, 0.2, 0.1])
    z1 = d.initialize(spec, position=[0, 0, 0.6], velocity=[0.0, 0.0, 0.0], angular_velocity=[0.0, 0.0, 0.0])
    Z = np.stack([z0, z1]); U = np.zeros((2, 6))
    for _ in range(4):
        r = emu_step(spec, Z, U, opts=TIGHT, envs_per_wave=2, quad=True)
        Zo = np.stack([o.step(Z[b], U[b])[0] for b in range(2)])
        assert np.abs(r["z_next"] - Zo).max() < 1e-7
        Z = Zo
    assert r["iters"][0] != r["iters"][1]        # different Newton iteration counts inside one wave


@pytest.mark.parametrize("cfg,pre,mode,quad", [(1, 2, 0, True), (2, 1, 1, True), (3, 0, 0, True), (3, 1, 1, True), (4, 4, 0, True), (5, 2, 0, True), (2, 1, 0, False)])
def test_gradients_match_oracle(cfg, pre, mode, quad):
    spec = d.baseline_config(cfg)
    opts = d.SolverOptions(rtol=1e-7, btol=1e-7)
    o = Oracle(spec, opts=opts)
    Z, U = d.synthetic_inputs(spec, 1)
    z, u = Z[0], U[0]
    for _ in range(pre):
        z, _ = o.step(z, u)
    o.step(z, u)
    dz, du = o.gradients(mode)
    r = emu_step(spec, z, u, opts=opts, grad=True, grad_mode=mode, quad=quad)
    assert np.abs(r["dz"][0] - dz).max() < 1e-6 * max(1.0, np.abs(dz).max())
    assert np.abs(r["du"][0] - du).max() < 1e-6 * max(1.0, np.abs(du).max())


def test_atlas_two_wavefront_quad_mapping():
    """31 bodies: one environment over two wavefronts' worth of lanes (128 emulated threads) -- the NW = 2 LDS layout,
    the contact-row pool by contact index and the workgroup reductions of the device source."""
    spec = d.baseline_config(5)
    opts = TIGHT
    o = Oracle(spec, opts=opts)
    Z, U = d.synthetic_inputs(spec, 1)
    zo, info = o.step(Z[0], U[0])
    r = emu_step(spec, Z[0], U[0], opts=opts, quad=True)
    assert r["status"][0] == info["status"] == 0
    assert np.abs(r["z_next"][0] - zo).max() < 1e-7


def test_contact_data_gradients_match_oracle():
    """get_contact_gradients (src/gradients/contact.jl): the contact-data columns [friction, radius, origin(3)] through the
    third kernel (re-uses the step kernel's hand-off), single-corner block sliding on the floor."""
    from dojo_amd.mechanisms import get_block
    spec = get_block(contact_corners=1)
    opts = d.SolverOptions(rtol=1e-8, btol=1e-8)
    o = Oracle(spec, opts=opts)
    z = d.initialize(spec, position=[0, 0, 0.0], velocity=[0.4, 0.2, 0.0], angular_velocity=[0.1, 0.0, 0.2])
    u = np.zeros(6)
    for _ in range(2):
        z, _ = o.step(z, u)
    for mode in (0, 1):
        o.step(z, u)
        dco = o.contact_gradients(mode)
        r = emu_step(spec, z, u, opts=opts, quad=True, grad=True, grad_mode=mode)
        assert np.abs(r["dc"][0] - dco).max() < 1e-7 * max(1.0, np.abs(dco).max())


def test_contact_data_gradients_ant():
    """the same for a tree (13 supernodes, four foot contacts on different bodies), Ant standing on the floor"""
    spec = d.baseline_config(3)
    opts = d.SolverOptions(rtol=1e-7, btol=1e-7)
    o = Oracle(spec, opts=opts)
    Z, U = d.synthetic_inputs(spec, 1)
    z, u = Z[0], U[0]
    for _ in range(12):
        z, _ = o.step(z, u)
    _, info = o.step(z, u)
    dco = o.contact_gradients(0)
    r = emu_step(spec, z, u, opts=opts, quad=True, grad=True, grad_mode=0)
    assert info["status"] == 0 and r["status"][0] == 0
    assert np.abs(r["dc"][0] - dco).max() < 1e-6 * max(1.0, np.abs(dco).max())


@pytest.mark.parametrize("cfg,pre,quad", [(1, 0, True), (2, 40, True), (4, 10, True), (2, 40, False)])
def test_storage_rows_match_oracle(cfg, pre, quad):
    """save_to_storage! rows (storage.jl:50-67): the device computes the momenta from the body residual of the solved
    step (dj::storage_row), the oracle from the joint impulses as momentum.jl:17-53 does."""
    spec = d.baseline_config(cfg)
    opts = d.SolverOptions(rtol=1e-10, btol=1e-10)
    o = Oracle(spec, opts=opts)
    Z, U = d.synthetic_inputs(spec, 1)
    z = Z[0].copy()
    for _ in range(pre):
        z, _ = o.step(z, U[0])
    S, st = o.simulate_storage(z, U[:1])
    r = emu_step(spec, z[None], U[:1], opts=opts, quad=quad)
    assert st[0] == 0 and r["status"][0] == 0
    assert np.abs(r["storage"][0] - S[0]).max() < 1e-9 * max(1.0, np.abs(S[0]).max())


@pytest.mark.parametrize("cfg,pre", [(2, 0), (4, 5)])
def test_external_force_matches_oracle(cfg, pre):
    """state.Fext / state.τext in the body residual (integrators/constraint.jl:15-18, set_external_force!
    bodies/set.jl:110-115), and the Storage row of a step with an external force (simulate! clears it before it records)."""
    import oracle as om
    from dojo_amd.quat import vrot
    spec = d.baseline_config(cfg)
    opts = d.SolverOptions(rtol=1e-10, btol=1e-10)
    o = Oracle(spec, opts=opts)
    Z, U = d.synthetic_inputs(spec, 1)
    z = Z[0].copy()
    for _ in range(pre):
        z, _ = o.step(z, U[0])
    rng = np.random.default_rng(1)
    F = rng.normal(size=(spec.Nb, 3)); Tq = rng.normal(size=(spec.Nb, 3)) * 0.1
    o.set_state(z)
    fe = np.zeros((spec.Nb, 6))
    for b in range(spec.Nb):
        o.set_external_force(b, force=F[b], torque=Tq[b])        # force in the body frame, as the reference takes it
        fe[b, :3] = vrot(F[b], z[13 * b + 6:13 * b + 10]); fe[b, 3:] = Tq[b]
    row = np.zeros((spec.Nb, 25))
    st = om.lib().orc_simulate_step_record(o.h, om._p(np.ascontiguousarray(U[0])), 1, om._p(row))
    r = emu_step(spec, z[None], U[:1], opts=opts, quad=True, fext=fe[None])
    assert st == 0 and r["status"][0] == 0
    assert np.abs(r["vel"][0] - o.velocity_solution()).max() < 1e-9
    assert np.abs(r["storage"][0] - row).max() < 1e-9 * max(1.0, np.abs(row).max())
    # and the force does change the step
    r0 = emu_step(spec, z[None], U[:1], opts=opts, quad=True)
    assert np.abs(r0["vel"][0] - r["vel"][0]).max() > 1e-4


@pytest.mark.parametrize("corners,quad", [(4, True), (8, True), (4, False)])
def test_impact_contact_matches_oracle(corners, quad):
    """ImpactContact (src/contacts/impact.jl).  The oracle implements it as the reference does (one γ and one s per contact,
    2x2 diagonal block, orthant line search, cone degree 1); the device runs the nonlinear rows with the friction block
    pinned at the neutral vector.  Same Newton iterates: equal iteration counts, states to round-off."""
    spec = d.get_block(contact_type="impact", contact_corners=corners)
    opts = d.SolverOptions(rtol=1e-9, btol=1e-9)
    o = Oracle(spec, opts=opts)
    z = d.initialize(spec, position=[0, 0, 0.05], velocity=[1.0, 0.5, -0.5], angular_velocity=[0.5, 0.2, 0.3])
    for k in range(8):
        zo, info = o.step(z, np.zeros(6))
        r = emu_step(spec, z[None], np.zeros((1, 6)), opts=opts, quad=quad)
        assert info["status"] == 0 and r["status"][0] == 0 and r["iters"][0] == info["iters"]
        assert np.abs(r["z_next"][0] - zo).max() < 1e-10
        sg = o.get_solution()[6:].reshape(corners, 2)                       # [s, γ] per contact
        csg = r["contact_sg"][0].reshape(corners, 8)
        assert np.abs(csg[:, 0] - sg[:, 0]).max() < 1e-9 and np.abs(csg[:, 4] - sg[:, 1]).max() < 1e-9
        assert np.array_equal(csg[:, 1:4], np.tile([1.0, 0, 0], (corners, 1)))   # the pinned friction block
        z = zo


@pytest.mark.parametrize("seed,quad", [(1, True), (2, True), (4, False), (6, True)])
def test_random_tree_mechanisms(seed, quad):
    """Random trees (tests/random_mechanisms.py): Revolute / Spherical / Fixed joints with random axes, vertices, offsets,
    springs, dampers and limits below a Floating root with contacts.  Equal iteration counts, states and both gradient
    conventions against the oracle."""
    from random_mechanisms import random_mechanism
    spec, z, u = random_mechanism(seed)
    opts = d.SolverOptions(rtol=1e-9, btol=1e-9)
    o = Oracle(spec, opts=opts)
    for k in range(2):
        zo, info = o.step(z, u)
        r = emu_step(spec, z[None], u[None], opts=opts, quad=quad, grad=(k == 1), grad_mode=k % 2)
        assert info["status"] == 0 and r["status"][0] == 0 and r["iters"][0] == info["iters"]
        assert np.abs(r["z_next"][0] - zo).max() < 1e-10
        if k == 1:
            dz, du = o.gradients(mode=1)
            assert np.abs(r["dz"][0] - dz).max() < 1e-8 * max(1.0, np.abs(dz).max())
            assert np.abs(r["du"][0] - du).max() < 1e-8 * max(1.0, np.abs(du).max())
        z = zo


TSD_CASES = [("slider", dict(springs=5.0, dampers=0.7)), ("nslider", dict(num_bodies=3, springs=4.0, dampers=0.5)),
             ("raiberthopper", dict()), ("raiberthopper", dict(springs=(0.0, 30.0), dampers=(0.0, 2.0)))]


@pytest.mark.parametrize("name,kw", TSD_CASES)
def test_translational_springs_dampers(name, kw):
    """Translational springs / dampers (translational/springs.jl, dampers.jl; the DJ_TSD path of the lane program) on the
    reference's slider, nslider and raiberthopper (its default has a damped Prismatic leg): equal Newton iteration counts
    (the damper's velocity Jacobian is exact), states and IFT Jacobians in both conventions to round-off."""
    spec = d.get_mechanism(name, **kw)
    opts = d.SolverOptions(rtol=1e-9, btol=1e-9)
    o = Oracle(spec, opts=opts)
    Z, U = d.synthetic_inputs(spec, 1)
    z, u = Z[0], U[0]
    for k in range(3):
        zo, info = o.step(z, u)
        r = emu_step(spec, z, u, opts=opts, quad=True, grad=True, grad_mode=k % 2)
        assert info["status"] == 0 and r["status"][0] == 0 and r["iters"][0] == info["iters"]
        assert np.abs(r["z_next"][0] - zo).max() < 1e-10
        dz, du = o.gradients(mode=k % 2)
        assert np.abs(r["dz"][0] - dz).max() < 1e-7 * max(1.0, np.abs(dz).max())
        assert np.abs(r["du"][0] - du).max() < 1e-7 * max(1.0, np.abs(du).max())
        z = zo


@pytest.mark.parametrize("seed", [100, 103, 104, 106])
def test_random_tree_mechanisms_with_translational_joints(seed):
    """Random trees that mix in Prismatic / Planar / Cylindrical / FixedOrientation joints with springs, dampers and spring
    offsets on their translational (and free rotational) coordinates."""
    from random_mechanisms import random_mechanism
    spec, z, u = random_mechanism(seed, translational=True)
    opts = d.SolverOptions(rtol=1e-9, btol=1e-9)
    o = Oracle(spec, opts=opts)
    for k in range(2):
        zo, info = o.step(z, u)
        r = emu_step(spec, z[None], u[None], opts=opts, quad=True, grad=True, grad_mode=k % 2)
        assert info["status"] == 0 and r["status"][0] == 0 and r["iters"][0] == info["iters"]
        assert np.abs(r["z_next"][0] - zo).max() < 1e-10
        dz, du = o.gradients(mode=k % 2)
        assert np.abs(r["dz"][0] - dz).max() < 1e-8 * max(1.0, np.abs(dz).max())
        assert np.abs(r["du"][0] - du).max() < 1e-8 * max(1.0, np.abs(du).max())
        z = zo


@pytest.mark.parametrize("joint_type", ["Prismatic", "Planar", "Cylindrical", "PlanarAxis", "Orbital", "PrismaticOrbital", "FreeOrbital", "CylindricalFree"])
def test_snake_joint_prototypes(joint_type):
    """The reference loops its damper / minimal-coordinate tests over every joint prototype on the snake (test/damper.jl:2-25,
    test/minimal.jl): the same mechanism with springs and dampers on the device program.  (All fifteen prototypes on snake,
    twister and npendulum run in the GPU tier.)"""
    spec = d.get_mechanism("snake", num_bodies=2, joint_type=joint_type, springs=1.0, dampers=0.3)
    opts = d.SolverOptions(rtol=1e-9, btol=1e-9)
    o = Oracle(spec, opts=opts)
    Z, U = d.synthetic_inputs(spec, 1)
    z, u = Z[0], U[0]
    zo, info = o.step(z, u)
    r = emu_step(spec, z, u, opts=opts, quad=True, grad=True, grad_mode=1)
    assert info["status"] == 0 and r["status"][0] == 0 and r["iters"][0] == info["iters"]
    assert np.abs(r["z_next"][0] - zo).max() < 1e-10
    dz, du = o.gradients(mode=1)
    assert np.abs(r["dz"][0] - dz).max() < 1e-7 * max(1.0, np.abs(dz).max())
    assert np.abs(r["du"][0] - du).max() < 1e-7 * max(1.0, np.abs(du).max())


def _limited(name):
    from dojo_amd.mechanisms import set_limits
    if name == "slider":
        return d.get_slider(joint_limits={"joint": [-0.2, 0.3]}, dampers=0.1, springs=0.5), 30, 6, None
    if name == "raiberthopper":
        spec = d.get_raiberthopper(timestep=0.01); set_limits(spec, {"leg": [-0.6, -0.4]})
        return spec, 12, 4, 30.0
    spec = d.get_twister(num_bodies=3, joint_type="Cylindrical", springs=0.5, dampers=0.2)
    for j in spec.joints[1:]:
        j.tra.limits = (np.array([-0.05]), np.array([0.08]))
    return spec, 9, 3, None


@pytest.mark.parametrize("name,quad", [("slider", True), ("slider", False), ("raiberthopper", True), ("twister", True)])
def test_translational_joint_limits(name, quad):
    """Limits on the translational coordinate of Prismatic-type joints (the Δκ row in the third translational slot, DJ_TSD
    builds): free, hitting the stop and resting on it -- iteration counts, states, exported (s, γ) and both gradient conventions."""
    spec, steps, every, push = _limited(name)
    opts = d.SolverOptions(rtol=1e-9, btol=1e-9)
    o = Oracle(spec, opts=opts)
    Z, U = d.synthetic_inputs(spec, 1)
    z, u = (d.initialize(spec), np.array([0.3])) if name == "slider" else (Z[0], U[0])
    if push is not None:
        u = u.copy(); u[-1] = push                    # drive the leg into its stop
    nj = spec.n_joint_impulses; active = 0.0
    for k in range(steps):
        zo, info = o.step(z, u)
        if k % every == every - 1:
            r = emu_step(spec, z, u, opts=opts, quad=quad, grad=True, grad_mode=k % 2)
            so = o.get_solution()
            assert info["status"] == 0 and r["status"][0] == 0 and r["iters"][0] == info["iters"]
            assert np.abs(r["z_next"][0] - zo).max() < 1e-10 and np.abs(r["joint_imp"][0] - so[:nj]).max() < 1e-8
            dz, du = o.gradients(mode=k % 2)
            assert np.abs(r["dz"][0] - dz).max() < 1e-6 * max(1.0, np.abs(dz).max())
            assert np.abs(r["du"][0] - du).max() < 1e-6 * max(1.0, np.abs(du).max())
            active = max(active, np.abs(so[:nj]).max())
        z = zo
    assert active > 1e-3                              # a limit impulse was active at one of the compared steps


@pytest.mark.parametrize("name,kw,pre", [("cartpole", dict(joint_limits={"cart_joint": [-0.3, 0.3]}, dampers=0.1), 0), ("block2d", dict(), 50),
                                         ("dzhanibekov", dict(), 5), ("tippetop", dict(), 10), ("sphere", dict(), 45)])
def test_more_reference_mechanisms(name, kw, pre):
    """cartpole (Prismatic cart with limits + Revolute pole), block2d (PlanarAxis root, four contacts), dzhanibekov, tippetop,
    sphere: the reference's builders from their nominal states, after `pre` oracle steps (contacts active where there are any)."""
    spec = d.get_mechanism(name, **kw)
    opts = d.SolverOptions(rtol=1e-9, btol=1e-9)
    o = Oracle(spec, opts=opts)
    z = d.initialize(spec); u = 0.3 * np.ones(spec.nu)
    if spec.joints[0].nu == 6:
        u[:6] = 0
    for _ in range(pre):
        z, _ = o.step(z, u)
    zo, info = o.step(z, u)
    r = emu_step(spec, z, u, opts=opts, quad=True, grad=True, grad_mode=1)
    assert info["status"] == 0 and r["status"][0] == 0 and r["iters"][0] == info["iters"]
    assert np.abs(r["z_next"][0] - zo).max() < 1e-10
    dz, du = o.gradients(mode=1)
    assert np.abs(r["dz"][0] - dz).max() < 1e-6 * max(1.0, np.abs(dz).max())
    assert np.abs(r["du"][0] - du).max() < 1e-6 * max(1.0, np.abs(du).max())


@pytest.mark.parametrize("cfg,pre", [(3, 6), (1, 2)])
def test_refining_kernels_match_oracle(cfg, pre):
    """The refining twins of the two kernels (dojo_stepp_kernel / dojo_gradp_kernel: iterative refinement of every Newton
    solve and of every IFT column against the uncondensed blocks) with every environment sent there (threshold 0, as
    dojo_set_refinement(h, 0) does), next to the plain kernels: the same iteration count as the oracle, and a refined
    gradient closer to the oracle's than 1e-7."""
    spec = d.baseline_config(cfg)
    o = Oracle(spec, opts=TIGHT)
    Z, U = d.synthetic_inputs(spec, 1)
    z, u = Z[0], U[0]
    for _ in range(pre):
        z, _ = o.step(z, u)
    zo, info = o.step(z, u)
    dz, du = o.gradients(0)
    r = emu_step(spec, z, u, opts=TIGHT, grad=True, quad=True, refine=0.0)
    p = emu_step(spec, z, u, opts=TIGHT, grad=True, quad=True, refine=float("inf"))
    assert r["status"][0] == info["status"] == 0 and r["iters"][0] == info["iters"]
    assert np.abs(r["z_next"][0] - zo).max() < 1e-9
    scale = max(1.0, np.abs(dz).max())
    assert np.abs(r["dz"][0] - dz).max() < 1e-7 * scale and np.abs(r["du"][0] - du).max() < 1e-7 * scale
    assert np.abs(p["dz"][0] - dz).max() < 1e-5 * scale        # the plain kernels: usable, not refined


@pytest.mark.parametrize("cfg,pre", [(3, 5), (2, 6)])
def test_fp32_abi_gradients_match_oracle(cfg, pre):
    """fp32 buffers at the ABI (the mode bench.py times): the state an fp32 buffer stands for has unit quaternions (normalized
    on load), the IFT parks its forward-substituted right-hand sides in an fp64 buffer of its own (KernelArgs::ypark) -- what
    is left against the oracle on that state is the rounding of the fp32 outputs."""
    spec = d.baseline_config(cfg)
    o = Oracle(spec)
    Z, U = d.synthetic_inputs(spec, 2)
    for _ in range(pre):
        Z = np.stack([o.step(Z[b], U[b])[0] for b in range(2)])
    Z32 = Z.astype(np.float32).astype(np.float64); U32 = U.astype(np.float32).astype(np.float64)
    r = emu_step(spec, Z32, U32, dtype="f32", grad=True, quad=True)
    for b in range(2):
        zo, info = o.step(d.fp32_abi_state(Z32[b]), U32[b])
        dz, du = o.gradients(0)
        assert r["status"][b] == info["status"] == 0 and r["iters"][b] == info["iters"]
        assert np.abs(r["z_next"][b] - zo).max() < 1e-5
        assert np.abs(r["dz"][b] - dz).max() < 1e-5 * max(1.0, np.abs(dz).max())
        if spec.nu:
            assert np.abs(r["du"][b] - du).max() < 1e-5 * max(1.0, np.abs(du).max())


@pytest.mark.parametrize("name,kw,v0", [("sphere", dict(), [1.0, 0.4, 0.0]), ("block", dict(contact_corners=4, friction_coefficient=0.3), [1.2, 0.9, 0.0]),
                                        ("block", dict(contact_corners=4, friction_coefficient=0.3), [0.0, 0.0, 0.0])])
def test_linear_contact_matches_oracle(name, kw, v0):
    """LinearContact (src/contacts/linear.jl; -DDJ_LINEAR builds of the device source: six orthant pairs [γ ψ β1..β4] per contact,
    condensed onto the body block through the same three directions as the nonlinear cone): free flight, impact, sliding along
    and across the pyramid's axes and rest, against the oracle -- equal Newton iteration counts, states, and all twelve
    exported cone variables of every contact."""
    spec = d.get_mechanism(name, contact_type="linear", **kw)
    o = Oracle(spec, opts=TIGHT)
    z = d.initialize(spec, position=[0, 0, 0.05], velocity=v0, angular_velocity=[0.3, -0.2, 0.5]) if name == "block" else d.initialize(spec)
    if name == "sphere":
        z = z.copy(); z[2] = 0.52; z[3:6] = v0; z[10:13] = [0.5, -1.0, 0.2]
    u = np.zeros(spec.nu)
    for k in range(14):
        zo, info = o.step(z, u)
        r = emu_step(spec, z, u, opts=TIGHT, quad=True)
        # (the impact step of the sphere runs into max_iter in the oracle as well: the iterate paths still agree to round-off)
        assert r["status"][0] == info["status"] and r["iters"][0] == info["iters"], (k, r["status"][0], info["status"], r["iters"][0], info["iters"])
        assert np.abs(r["z_next"][0] - zo).max() < 1e-8, (k, np.abs(r["z_next"][0] - zo).max())
        sg = o.get_solution()[6 * spec.Nb + spec.n_joint_impulses:]
        assert np.abs(r["contact_sg"][0] - sg).max() < 1e-7 * max(1.0, np.abs(sg).max()), k
        z = zo
    assert (sg.reshape(-1, 12)[:, 6] > 1e-4).any()                  # in contact by the end


@pytest.mark.parametrize("name,kw", [("snake", dict(num_bodies=3)), ("twister", dict(num_bodies=3))])
def test_linear_contact_on_articulated_mechanisms(name, kw):
    """LinearContact on several bodies of a tree (two contacts per snake link: the MAXC = 4 LinearContact build; joints and
    contacts in one supernode): actuated free fall and landing against the oracle, equal iterate paths and states."""
    spec = d.get_mechanism(name, contact_type="linear", **kw)
    o = Oracle(spec, opts=TIGHT)
    z = d.initialize(spec); u = 0.2 * np.ones(spec.nu)
    touched = False
    for k in range(60):
        zo, info = o.step(z, u)
        if k % 3 == 0 or touched:
            r = emu_step(spec, z, u, opts=TIGHT, quad=True)
            assert r["status"][0] == info["status"] and r["iters"][0] == info["iters"], (k, r["iters"][0], info["iters"])
            assert np.abs(r["z_next"][0] - zo).max() < 1e-8, (k, np.abs(r["z_next"][0] - zo).max())
        sg = o.get_solution()[6 * spec.Nb + spec.n_joint_impulses:].reshape(-1, 12)
        touched = touched or bool((sg[:, 6] > 1e-4).any())
        z = zo
        if touched and k > 45:
            break
    assert touched


def test_ift_hard_cases_lu_form():
    """The IFT on the environment-steps where the explicit-inverse sweeps lost their digits (tests/golden/hard_cases_ant.npz: Ant states a
    GPU hunt over 4096 x 9 environment-steps dumped, reference-default tolerances; a foot in sticking contact behind its Fixed joint, max
    gamma/s 1e6 .. 1e8).  With the products by the explicitly inverted supernode blocks the gradients of these were off by up to 1.8e-5
    relative; the LU form of the tree elimination (factorize_quad_lu) brings every one within 1e-7."""
    G_ = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hard_cases_ant.npz"))
    order = np.argsort(-G_["meta"][:, 3])[:8]
    Z, U = G_["z"][order], G_["u"][order]
    spec = d.baseline_config(3)
    o = Oracle(spec)
    Zo, st_o, it_o, dz_o, du_o = o.step_batch(Z, U, with_grad=True, nthreads=4)
    r = emu_step(spec, Z, U, grad=True, quad=True)
    assert np.array_equal(r["status"], st_o) and np.array_equal(r["iters"], it_o)
    n_cmp = 0
    for b in range(len(Z)):
        if np.abs(r["z_next"][b] - Zo[b]).max() > 1e-9:       # (one 34-iteration solve of the set ends 8e-6 away from the oracle's: different points, different Jacobians)
            assert it_o[b] > 20
            continue
        n_cmp += 1
        assert np.abs(r["dz"][b] - dz_o[b]).max() <= 1e-7 * max(1.0, np.abs(dz_o[b]).max())
        assert np.abs(r["du"][b] - du_o[b]).max() <= 1e-7 * max(1.0, np.abs(du_o[b]).max())
    assert n_cmp >= 7


def test_ift_f32_abi_constraint_rows_in_double():
    """fp32 ABI: the eight environments of the BASELINE Ant batch whose gradients were furthest off (tools/hunt_f32.py on the GPU: up to
    1.4e-5 relative; tests/golden/hard_cases_ant_f32.npz).  The cause was the fp32 rounding of the IFT's right-hand sides on the JOINT rows
    and the joint-limit slack rows (constraint rows: amplified by 1/dt and more on their way to the velocities); those blocks are double
    now (QuadRhs::jd) and what is left is the rounding of the fp32 output, < 1e-7."""
    G_ = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hard_cases_ant_f32.npz"))
    Z, U = G_["z"][:4], G_["u"][:4]
    spec = d.baseline_config(3)
    o = Oracle(spec)
    Zo, st_o, it_o, dz_o, du_o = o.step_batch(d.fp32_abi_state(Z), U, with_grad=True, nthreads=4)
    r = emu_step(spec, Z, U, grad=True, quad=True, dtype="f32")
    assert np.array_equal(r["status"], st_o) and np.array_equal(r["iters"], it_o)
    for b in range(len(Z)):
        assert G_["eg"][b] > 2e-6                                   # (what the kernels of round 2 gave on this environment)
        assert np.abs(r["dz"][b] - dz_o[b]).max() <= 1e-7 * max(1.0, np.abs(dz_o[b]).max())
        assert np.abs(r["du"][b] - du_o[b]).max() <= 1e-7 * max(1.0, np.abs(du_o[b]).max())


@pytest.mark.parametrize("seed,nb", [(3052, 36), (5015, 33), (5018, 40)])
def test_lane_per_supernode_mapping_lu_form(seed, nb):
    """Mechanisms above 32 bodies run one lane per supernode.  With products by an explicitly inverted 12x12 supernode block that
    mapping took up to twice the oracle's iterations on about one random tree in ten and ran out of iterations on some at 1e-9
    (a GPU sweep found seed 3052; 5015 and 5018 are from the emulator survey); with the supernode blocks LU-factorized and
    triangular solves (LaneProgram::factorize / core_solve) iteration counts and states are the oracle's at 1e-9, and the gradients
    at the reference's default tolerances (this mapping has no refining kernels: at 1e-9 its IFT keeps the ~1e-6 of the condensed
    cone rows)."""
    from random_mechanisms import random_mechanism
    spec, z0, u0 = random_mechanism(seed, nb=nb, contact_type="nonlinear", translational=False, tra_limits=False)
    rng = np.random.default_rng(seed)
    Z = np.tile(z0, (2, 1)); U = np.tile(u0, (2, 1)) + rng.normal(size=(2, spec.nu)) * 0.2
    for tol in (1e-9, None):
        opts = d.SolverOptions(rtol=tol, btol=tol) if tol else d.SolverOptions()
        o = Oracle(spec, opts=opts)
        r = emu_step(spec, Z, U, opts=opts, quad=False, grad=tol is None)
        for b in range(2):
            zo, info = o.step(Z[b], U[b])
            assert info["status"] == 0 and r["status"][b] == 0 and r["iters"][b] == info["iters"]
            assert np.abs(r["z_next"][b] - zo).max() < 1e-9
            if tol is None:
                dz, du = o.gradients(mode=0)
                assert np.abs(r["dz"][b] - dz).max() < 1e-7 * max(1.0, np.abs(dz).max())
                assert np.abs(r["du"][b] - du).max() < 1e-7 * max(1.0, np.abs(du).max())


def _two_sphere_state(x1, x2, v2, w2=(0, 0, 0), v1=(0, 0, 0)):
    z = np.zeros((2, 13)); z[:, 6] = 1.0
    z[0, 0:3] = x1; z[0, 3:6] = v1; z[1, 0:3] = x2; z[1, 3:6] = v2; z[1, 10:13] = w2
    return z.reshape(-1)


SS_CASES = [(-9.81, "Fixed", [0, 0, 2.0], [0, 0, 0], (0, 0, 0)), (0.0, "Fixed", [0, 0, 2.0], [0, 0, -5.0], (0, 0, 0)), (0.0, "Floating", [0, 0, 2.0], [0, 0, -5.0], (0, 0, 0)),
            (0.0, "Fixed", [2.0, 0, 0], [-5.0, 0, 0], (0, 0, 0)), (-9.81, "Floating", [0.3, 0.1, 1.5], [0.5, 0.2, -1.0], (1.0, -2.0, 0.5))]


@pytest.mark.parametrize("friction_type", ["nonlinear", "impact", "linear"])
def test_body_body_contact_matches_oracle(friction_type):
    """SphereSphereCollision between a body and its tree child (src/contacts/collisions/sphere_sphere.jl; the two-sphere mechanism of
    test/collisions.jl:2-58): the rollouts of the reference's test -- resting under gravity, thrown at the fixed sphere, at a floating one,
    along x -- and a spinning off-axis landing on a floating sphere.  Same Newton iterates as the oracle: equal iteration counts, states
    and contact variables to round-off (the contact rows couple the child's supernode to its parent's: U, L and Dup blocks)."""
    for g, joint, x2, v2, w2 in SS_CASES:
        spec = d.get_two_spheres(friction_type=friction_type, gravity=g, joint_world_body1=joint)
        o = Oracle(spec)
        z = _two_sphere_state([0, 0, 0], x2, v2, w2)
        for k in range(20):
            zo, info = o.step(z, np.zeros(spec.nu))
            r = emu_step(spec, z[None], np.zeros((1, spec.nu)), quad=True)
            assert info["status"] == 0 and r["status"][0] == 0 and r["iters"][0] == info["iters"]
            assert np.abs(r["z_next"][0] - zo).max() < (1e-7 if friction_type == "linear" else 1e-9)      # (LinearContact: 1e-8, as on a half-space)
            nh = {"impact": 1, "nonlinear": 4, "linear": 6}[friction_type]; per = 6 if friction_type == "linear" else 4
            sg = o.get_solution()[-2 * nh:]
            csg = r["contact_sg"][0]
            assert np.abs(csg[0:nh] - sg[:nh]).max() < 1e-7 and np.abs(csg[per:per + nh] - sg[nh:]).max() < 1e-7
            z = zo


@pytest.mark.parametrize("contact_type", ["linear", "impact"])
def test_storage_rows_with_the_other_contact_models(contact_type):
    """save_to_storage! for LinearContact and ImpactContact mechanisms: dj::storage_row takes the contact impulses from the exported cone
    variables with the model's own force mapping (contact_impulses); a block sliding on the floor, against the oracle's momentum.jl restatement"""
    spec = d.get_block(contact_type=contact_type, contact_corners=4, friction_coefficient=0.3)
    o = Oracle(spec)
    z = d.initialize(spec, position=[0, 0, 0.02], velocity=[1.2, 0.9, -0.3], angular_velocity=[0.3, -0.2, 0.5])
    pressed = False
    for k in range(8):
        S, st = o.simulate_storage(z, np.zeros((1, spec.nu)))
        r = emu_step(spec, z[None], np.zeros((1, spec.nu)), quad=True)
        assert st[0] == 0 and r["status"][0] == 0
        assert np.abs(r["storage"][0] - S[0]).max() < 1e-8 * max(1.0, np.abs(S[0]).max())
        nh = 6 if contact_type == "linear" else 1
        pressed = pressed or o.get_solution()[6:].reshape(4, 2 * nh)[:, nh].max() > 1e-3
        z, _ = o.step(z, np.zeros(spec.nu))
    assert pressed


def test_body_body_contact_storage_rows():
    """save_to_storage! with a body-body contact: the momenta of BOTH bodies need the contact impulse (dj::storage_row evaluates the
    contact from either side with the partner's state); against the oracle's momentum.jl restatement, in contact"""
    spec = d.get_two_spheres(friction_type="nonlinear", gravity=-9.81, joint_world_body1="Floating")
    opts = d.SolverOptions()
    o = Oracle(spec, opts=opts)
    z = _two_sphere_state([0, 0, 0], [0.2, 0.1, 1.05], [0.3, 0.0, -2.0], (0.5, 1.0, 0.0))
    hit = False
    for k in range(6):
        S, st = o.simulate_storage(z, np.zeros((1, spec.nu)))
        r = emu_step(spec, z[None], np.zeros((1, spec.nu)), opts=opts, quad=True)
        assert st[0] == 0 and r["status"][0] == 0
        assert np.abs(r["storage"][0] - S[0]).max() < 1e-9 * max(1.0, np.abs(S[0]).max())
        hit = hit or o.get_solution()[-4] > 1e-3
        z, _ = o.step(z, np.zeros(spec.nu))
    assert hit


def test_body_body_contact_in_a_chain_with_a_half_space_contact():
    """a pendulum bob (Revolute to the world) carrying a free sphere that also touches the floor plane through a half-space contact of its
    own... the free sphere owns the body-body contact, the bob a half-space contact: both kinds in one mechanism, one contact per body"""
    from dojo_amd.mechanisms import BodySpec, MechanismSpec, Revolute, Floating, sphere_inertia, contact_constraint, sphere_sphere_contact
    bodies = [BodySpec("bob", 2.0, sphere_inertia(0.3, 2.0)), BodySpec("ball", 0.5, sphere_inertia(0.2, 0.5))]
    joints = [Revolute("pin", -1, 0, np.array([1.0, 0, 0]), child_vertex=np.array([0, 0, 0.8])), Floating("free", 0, 1)]
    contacts = [contact_constraint("floor", 0, np.array([0, 0, 1.0]), 0.6, contact_radius=0.3, contact_offset=np.array([0, 0, -1.2])),
                sphere_sphere_contact("touch", 0, 1, 0.3, 0.2, 0.4)]
    spec = MechanismSpec("bob_and_ball", bodies, joints, contacts, 0.02, None, np.array([0.0, 0.0, -9.81]))
    o = Oracle(spec)
    z = np.zeros((2, 13)); z[:, 6] = 1.0
    z[0, 0:3] = [0, 0, -0.8]; z[1, 0:3] = [0.05, 0.1, -0.25]; z[1, 3:6] = [0, 0.3, -0.5]; z[0, 10:13] = [0.4, 0, 0]
    z = z.reshape(-1)
    touched = False
    for k in range(40):
        zo, info = o.step(z, np.zeros(spec.nu))
        r = emu_step(spec, z[None], np.zeros((1, spec.nu)), quad=True)
        assert info["status"] == 0 and r["status"][0] == 0 and abs(int(r["iters"][0]) - info["iters"]) == 0
        assert np.abs(r["z_next"][0] - zo).max() < 1e-9
        touched = touched or o.get_solution()[-4] > 1e-4
        z = zo
    assert touched


def test_body_body_contacts_in_a_stack_of_three_spheres():
    """a chain of body-body contacts: three spheres, the lowest on the floor (half-space contact), each next one touching the one below through a
    SphereSphereCollision contact and hanging in the tree on it; dropped slightly off-axis, the stack settles and then topples.  Equal Newton
    iteration counts with the oracle on every step but at most one long solve at the impact (see below); states to 1e-5"""
    from dojo_amd.mechanisms import BodySpec, MechanismSpec, Floating, sphere_inertia, contact_constraint, sphere_sphere_contact
    r = 0.3
    bodies = [BodySpec("s%d" % i, 1.0, sphere_inertia(r, 1.0)) for i in range(3)]
    joints = [Floating("j0", -1, 0), Floating("j1", 0, 1), Floating("j2", 1, 2)]
    contacts = [contact_constraint("floor", 0, np.array([0, 0, 1.0]), 0.8, contact_radius=r),
                sphere_sphere_contact("c01", 0, 1, r, r, 0.8), sphere_sphere_contact("c12", 1, 2, r, r, 0.8)]
    spec = MechanismSpec("stack", bodies, joints, contacts, 0.02, None, np.array([0.0, 0.0, -9.81]))
    o = Oracle(spec)
    z = np.zeros((3, 13)); z[:, 6] = 1.0
    z[0, 0:3] = [0, 0, r + 0.05]; z[1, 0:3] = [0.01, 0.0, 3 * r + 0.1]; z[2, 0:3] = [0.0, 0.01, 5 * r + 0.15]
    z = z.reshape(-1)
    carried = False; stalled = 0
    for k in range(40):
        zo, info = o.step(z, np.zeros(spec.nu))
        rr = emu_step(spec, z[None], np.zeros((1, spec.nu)), quad=True)
        assert info["status"] == 0
        if rr["iters"][0] > 20 and rr["iters"][0] != info["iters"]:
            # A LONG solve on the device (the criterion of DESIGN.md section 7): at the impact of the stack the Newton matrix of the body-body
            # contacts is inexact by construction (as the reference's), mu runs to 1e-20 and the condensed solve leaves a residual floor of
            # ~1.5e-6 against rtol = 1e-6 -- the device runs into max_iter where the oracle's pivoted, refined LU gets through in 12.
            # Which step this is depends on the last bits of the trajectory; it may happen once, and the states still agree to 1e-4.
            stalled += 1
            assert rr["status"][0] in (0, 1), rr["status"]           # converged late, or max_iter: nothing else (never the ω-clipping status)
            print("stack of three spheres: device solve of step %d took %d iterations (oracle %d), status %d, state %.2e apart" % (k, rr["iters"][0], info["iters"], rr["status"][0], np.abs(rr["z_next"][0] - zo).max()))
            assert np.abs(rr["z_next"][0] - zo).max() < 1e-4
        else:
            assert rr["status"][0] == 0 and rr["iters"][0] == info["iters"]
            assert np.abs(rr["z_next"][0] - zo).max() < 1e-5
        g = o.get_solution()[-24:].reshape(3, 8)[:, 4]
        carried = carried or (g[1] > 0.05 and g[2] > 0.05)          # both upper contacts loaded at the same time
        z = zo
    assert carried and stalled <= 1


def _rotm(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def off_centre_pair(friction_type, joint):
    """two boxes carrying contact spheres OFF their centres of mass (origin_parent, origin_child != 0: the sphere centres move with the bodies'
    rotations), the first on a Floating or Revolute joint to the world; the second approaches with spin, 0.02 from touching"""
    from dojo_amd.mechanisms import BodySpec, MechanismSpec, Floating, Revolute, box_inertia, sphere_sphere_contact
    op, oc = np.array([0.15, -0.05, 0.1]), np.array([-0.1, 0.05, -0.15])
    bodies = [BodySpec("a", 2.0, box_inertia(0.6, 0.4, 0.3, 2.0)), BodySpec("b", 0.7, box_inertia(0.3, 0.3, 0.5, 0.7))]
    j0 = Floating("j0", -1, 0) if joint == "Floating" else Revolute("j0", -1, 0, np.array([0, 1.0, 0]), child_vertex=np.array([0, 0, 0.4]))
    contacts = [sphere_sphere_contact("touch", 0, 1, 0.25, 0.2, 0.5, friction_type, origin_parent=op, origin_child=oc)]
    spec = MechanismSpec("off_centre", bodies, [j0, Floating("free", 0, 1)], contacts, 0.02, None, np.array([0.0, 0.0, -9.81]))
    rng = np.random.default_rng(3)
    z = np.zeros((2, 13)); z[:, 6] = 1.0
    qa = rng.normal(size=4); qa /= np.linalg.norm(qa); qb = rng.normal(size=4); qb /= np.linalg.norm(qb)
    z[0, 0:3] = [0, 0, -0.4] if joint == "Revolute" else [0, 0, 0]
    if joint == "Floating":
        z[0, 6:10] = qa
    z[1, 6:10] = qb
    dirv = np.array([0.3, -0.2, 1.0]); dirv /= np.linalg.norm(dirv)
    z[1, 0:3] = z[0, 0:3] + _rotm(z[0, 6:10]) @ op + dirv * 0.47 - _rotm(qb) @ oc
    z[1, 3:6] = -dirv + [0.2, 0.1, 0]; z[1, 10:13] = [1.0, -2.0, 0.5]; z[0, 10:13] = [0.3, 0.5, -0.2] if joint == "Floating" else [0, 0.4, 0]
    return spec, z.reshape(-1)


@pytest.mark.parametrize("friction_type", ["nonlinear", "impact", "linear"])
@pytest.mark.parametrize("joint", ["Floating", "Revolute"])
def test_body_body_contact_off_the_centres_of_mass(friction_type, joint):
    """SphereSphereCollision with origin_parent, origin_child != 0 (sphere_sphere.jl:11-16): the distance, the normal, the tangents and the contact
    points depend on both orientations -- the ω columns of the contact rows, the (v, ω) blocks of −∂(impulse)/∂(v, ω) and the reference's literal
    ∂t1ᵀ/∂q (collision.jl:207) come into play.  Equal Newton iterates with the oracle through approach, impact and sliding; Storage rows too."""
    spec, z = off_centre_pair(friction_type, joint)
    o = Oracle(spec)
    nh = {"impact": 1, "nonlinear": 4, "linear": 6}[friction_type]
    hit = False
    for k in range(15):
        S, st = o.simulate_storage(z, np.zeros((1, spec.nu)))
        zo, info = o.step(z, np.zeros(spec.nu))
        r = emu_step(spec, z[None], np.zeros((1, spec.nu)), quad=True)
        assert info["status"] == 0 and r["status"][0] == 0 and r["iters"][0] == info["iters"]
        assert np.abs(r["z_next"][0] - zo).max() < 1e-8
        assert np.abs(r["storage"][0] - S[0]).max() < 1e-8 * max(1.0, np.abs(S[0]).max())
        hit = hit or o.get_solution()[-nh] > 1e-3
        z = zo
    assert hit


def test_body_body_contact_inside_the_ant():
    """a body-body contact inside a BASELINE mechanism: a ball dropped on the Ant's front left leg link (fourteen bodies, the ball hangs in the tree
    on the link; the four foot contacts stay half-space contacts).  Status and Newton iteration counts equal to the oracle's on every step --
    including the steps where the reference's algorithm runs into max_iter on this contact on both sides -- and states to 1e-7 where it converges"""
    import copy
    from dojo_amd.mechanisms import BodySpec, Floating, sphere_inertia, sphere_sphere_contact
    base = d.baseline_config(3)
    spec = copy.deepcopy(base)
    link = 1                                                    # front_left_leg
    spec.bodies.append(BodySpec("ball", 0.3, sphere_inertia(0.1, 0.3)))
    spec.joints.append(Floating("ball_free", link, spec.Nb - 1))
    spec.contacts.append(sphere_sphere_contact("ball_on_leg", link, spec.Nb - 1, 0.1, 0.1, 0.6))
    Z0, U0 = d.synthetic_inputs(base, 1)
    zb = np.zeros(13); zb[6] = 1.0
    zb[0:3] = Z0[0][13 * link:13 * link + 3] + np.array([0.02, 0.01, 0.21]); zb[3:6] = Z0[0][13 * link + 3:13 * link + 6]
    z = np.concatenate([Z0[0], zb]); u = np.concatenate([U0[0], np.zeros(6)])
    o = Oracle(spec)
    loaded = False
    for k in range(10):
        zo, info = o.step(z, u)
        r = emu_step(spec, z[None], u[None], quad=True)
        assert r["status"][0] == info["status"] and r["iters"][0] == info["iters"]
        if info["status"] == 0:
            assert np.abs(r["z_next"][0] - zo).max() < 1e-7
        loaded = loaded or o.get_solution()[-4] > 1e-2
        z = zo
    assert loaded


@pytest.mark.parametrize("friction_type", ["nonlinear", "impact"])
def test_body_body_contact_between_free_bodies(friction_type):
    """SphereSphereCollision between two bodies that are NO tree neighbours (the reference's get_two_body: the second sphere has no joint at all,
    test/collisions.jl:2-58; here both spheres hang on the origin): the contact is a cut element of the general lane-mapping builds
    (LaneProgram::cut_contacts_M: the other body's rows through the low-rank correction of the tree solve).  The same cases as the tree-edge
    version above: equal status and Newton iteration counts with the oracle on every step, states to 1e-9, cone variables and Storage rows to 1e-8"""
    nh = {"impact": 1, "nonlinear": 4}[friction_type]
    for g, joint, x2, v2, w2 in SS_CASES:
        spec = d.get_two_spheres(friction_type=friction_type, gravity=g, joint_world_body1=joint, free_on="world")
        o = Oracle(spec)
        z = _two_sphere_state([0, 0, 0], x2, v2, w2)
        hit = False
        for k in range(20):
            S, st = o.simulate_storage(z, np.zeros((1, spec.nu)))
            zo, info = o.step(z, np.zeros(spec.nu))
            r = emu_step(spec, z[None], np.zeros((1, spec.nu)), quad=False)
            assert r["status"][0] == info["status"] == 0 and r["iters"][0] == info["iters"], (joint, k)
            assert np.abs(r["z_next"][0] - zo).max() < 1e-9
            assert np.abs(r["storage"][0] - S[0]).max() < 1e-8 * max(1.0, np.abs(S[0]).max())       # (momenta: the contact impulse on both spheres, found by ContactP::pbody)
            sg = o.get_solution()[-2 * nh:]; csg = r["contact_sg"][0]
            assert np.abs(csg[0:nh] - sg[:nh]).max() < 1e-8 and np.abs(csg[4:4 + nh] - sg[nh:]).max() < 1e-8
            hit = hit or sg[nh] > 1e-3
            z = zo
        assert hit


def folded_chain(friction_type="nonlinear", r=0.2, spread=None):
    """a three-link pendulum folded into a triangle, spheres on its first and last link: a body-body contact between two bodies of the SAME tree
    that are no neighbours (the cut element's H has the coupling of the two bodies through the tree).  spread: a random generator -> perturbed copy"""
    from dojo_amd.mechanisms import sphere_sphere_contact
    from dojo_amd.coords import minimal_state_dict, minimal_to_maximal
    spec = d.get_npendulum(num_bodies=3, timestep=0.01, dampers=0.1)
    spec.contacts.append(sphere_sphere_contact("first_on_last", 0, 2, r, r, 0.5, friction_type))
    a = np.array([0.3, 2.15, 2.15]); v = np.array([0.0, 0.5, 1.5])
    if spread is not None:
        a = a + 0.05 * spread.standard_normal(3); v = v + 0.3 * spread.standard_normal(3)
    x = minimal_state_dict(spec, coords={"joint:%d" % (i + 1): [a[i]] for i in range(3)}, vels={"joint:%d" % (i + 1): [v[i]] for i in range(3)})
    return spec, minimal_to_maximal(spec, x)


@pytest.mark.parametrize("friction_type", ["nonlinear", "impact"])
def test_body_body_contact_between_the_ends_of_a_chain(friction_type):
    """a cut contact inside ONE tree: the first and the last link of a folded three-link pendulum touch (no tree neighbours: the middle link sits
    between them).  Approach, impact -- one step on which the reference's algorithm runs into max_iter on both sides --, sliding contact and
    release: status and Newton iteration counts equal to the oracle's on every step, states to 1e-8"""
    spec, z = folded_chain(friction_type)
    o = Oracle(spec)
    nh = {"impact": 1, "nonlinear": 4}[friction_type]
    loaded = 0
    for k in range(25):
        zo, info = o.step(z, np.zeros(spec.nu))
        r = emu_step(spec, z[None], np.zeros((1, spec.nu)), quad=False)
        assert r["status"][0] == info["status"] and r["iters"][0] == info["iters"], k
        assert np.abs(r["z_next"][0] - zo).max() < 1e-8
        loaded += o.get_solution()[-nh] > 1e-2
        z = zo
    assert loaded >= 5


@pytest.mark.parametrize("seed", [0, 1, 2, 15, 85, 20])
def test_random_mechanisms_with_a_cut_element(seed):
    """tools/random_cut_sweep.py on a handful of its seeds (two per kind: a loop-closing Spherical joint between two random bodies of a random tree,
    a free ball thrown at a body, a contact between two bodies of the tree that are no neighbours): status, iteration counts and states equal to
    the oracle's over six steps, the IFT Jacobians of the loops on the last one"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    from random_cut_sweep import run
    msg, worst = run(seed)
    assert msg.endswith(" ok"), msg


def _ball_on_the_ant(free):
    """the Ant with a ball above its front left leg link: free = True: the ball is a free body (Floating joint to the origin; its contact with the
    link is no tree edge), False: it hangs in the tree on the link"""
    import copy
    from dojo_amd.mechanisms import BodySpec, Floating, sphere_inertia, sphere_sphere_contact
    base = d.baseline_config(3)
    spec = copy.deepcopy(base)
    link = 1                                                    # front_left_leg
    spec.bodies.append(BodySpec("ball", 0.3, sphere_inertia(0.1, 0.3)))
    spec.joints.append(Floating("ball_free", -1 if free else link, spec.Nb - 1))
    spec.contacts.append(sphere_sphere_contact("ball_on_leg", link, spec.Nb - 1, 0.1, 0.1, 0.6))
    Z0, U0 = d.synthetic_inputs(base, 1)
    zb = np.zeros(13); zb[6] = 1.0
    zb[0:3] = Z0[0][13 * link:13 * link + 3] + np.array([0.02, 0.01, 0.21]); zb[3:6] = Z0[0][13 * link + 3:13 * link + 6]
    return spec, np.concatenate([Z0[0], zb]), np.concatenate([U0[0], np.zeros(6)])


def test_free_ball_on_the_ant():
    """a cut contact inside a BASELINE mechanism: a FREE ball dropped on the Ant's front left leg link (fourteen bodies, two trees: the Ant and the
    ball; the four foot contacts stay half-space contacts of the tree).  Status and Newton iteration counts equal to the oracle's on every step,
    states to 1e-7 where it converges"""
    spec, z, u = _ball_on_the_ant(True)
    o = Oracle(spec)
    loaded = False
    for k in range(10):
        zo, info = o.step(z, u)
        r = emu_step(spec, z[None], u[None], quad=False)
        assert r["status"][0] == info["status"] and r["iters"][0] == info["iters"]
        if info["status"] == 0:
            assert np.abs(r["z_next"][0] - zo).max() < 1e-7
        loaded = loaded or o.get_solution()[-4] > 1e-2
        z = zo
    assert loaded


def test_a_loop_and_a_free_body_contact_together():
    """two cut elements of different kinds in one mechanism: the four-bar linkage (a loop-closing Revolute joint) and a free ball that falls on its
    coupler link (a body-body contact between bodies of different trees): one small system with a joint block and a contact block.  Equal Newton
    iterates with the oracle through approach, impact and rebound"""
    import copy
    from dojo_amd.mechanisms import BodySpec, Floating, sphere_inertia, sphere_sphere_contact
    base = d.get_fourbar()
    spec = copy.deepcopy(base)
    Z0, U0 = d.synthetic_inputs(base, 1)
    link = 1
    spec.bodies.append(BodySpec("ball", 0.2, sphere_inertia(0.05, 0.2)))
    spec.joints.append(Floating("ball_free", -1, spec.Nb - 1))
    spec.contacts.append(sphere_sphere_contact("ball_on_link", link, spec.Nb - 1, 0.05, 0.05, 0.5))
    zb = np.zeros(13); zb[6] = 1.0
    zb[0:3] = Z0[0][13 * link:13 * link + 3] + np.array([0.0, 0.01, 0.13]); zb[3:6] = Z0[0][13 * link + 3:13 * link + 6] + np.array([0, 0, -1.5])     # thrown at the link
    z = np.concatenate([Z0[0], zb]); u = np.concatenate([U0[0], np.zeros(6)])
    o = Oracle(spec)
    loaded = False
    for k in range(8):
        zo, info = o.step(z, u)
        r = emu_step(spec, z[None], u[None], quad=False)
        assert r["status"][0] == info["status"] == 0 and r["iters"][0] == info["iters"], k
        assert np.abs(r["z_next"][0] - zo).max() < 1e-8
        loaded = loaded or o.get_solution()[-4] > 1e-2
        z = zo
    assert loaded


@pytest.mark.parametrize("mode", [0, 1])
def test_gradients_of_a_forest(mode):
    """Several trees in one mechanism (bodies hanging on the origin independently): a two-link pendulum, a free sphere with a floor contact, and
    a single damped link.  The IFT sweeps are scheduled by branch with the ROOTS handled apart (their substitutions dealt out over all quads,
    their body rows' solution posted per root): three roots, one of them with a branch below it, control batches that span trees.  State and
    control Jacobians and the contact-data Jacobian against the oracle."""
    from random_mechanisms import forest_mechanism
    spec = forest_mechanism()
    opts = d.SolverOptions(rtol=1e-8, btol=1e-8)
    o = Oracle(spec, opts=opts)
    from random_mechanisms import forest_state
    z, u = forest_state(spec, o)
    zo, info = o.step(z, u)
    dz, du = o.gradients(mode); dc = o.contact_gradients(mode)
    r = emu_step(spec, z, u, opts=opts, grad=True, grad_mode=mode, quad=True)
    assert r["status"][0] == 0 and r["iters"][0] == info["iters"] and np.abs(r["z_next"][0] - zo).max() < 1e-9
    assert np.abs(r["dz"][0] - dz).max() < 1e-6 * max(1.0, np.abs(dz).max())
    assert np.abs(r["du"][0] - du).max() < 1e-6 * max(1.0, np.abs(du).max())
    assert np.abs(r["dc"][0] - dc).max() < 1e-6 * max(1.0, np.abs(dc).max())
    assert np.abs(dz[24:36, 0:24]).max() == 0 and np.abs(dc[0:24]).max() == 0          # (the trees do not talk to each other)


@pytest.mark.parametrize("name,kw", [("nslider", dict(num_bodies=20, springs=1.0, dampers=0.2)), ("snake", dict(num_bodies=18, joint_type="PlanarAxis", springs=1.0, dampers=0.3))])
def test_translational_springs_dampers_beyond_sixteen_bodies(name, kw):
    """Translational springs / dampers on mechanisms of more than 16 bodies: the lane mapping (one lane per supernode) evaluates them too
    (the product routes such mechanisms there, dojo_hip.hip mapping_waves; the two-wavefront quad mapping has no DJ_TSD build and the
    emulator refuses it like the product) -- states, iteration counts and IFT Jacobians against the oracle."""
    spec = d.get_mechanism(name, **kw)
    opts = d.SolverOptions(rtol=1e-9, btol=1e-9)
    Z, U = d.synthetic_inputs(spec, 2)
    o = Oracle(spec, opts=opts)
    r = emu_step(spec, Z, U, opts=opts, quad=False, grad=True, grad_mode=1)
    for b in range(2):
        zo, info = o.step(Z[b], U[b]); gz, gu = o.gradients(1)
        assert r["status"][b] == 0 and info["status"] == 0 and r["iters"][b] == info["iters"]
        assert np.abs(r["z_next"][b] - zo).max() < 1e-9
        assert np.abs(r["dz"][b] - gz).max() <= 1e-6 * max(1.0, np.abs(gz).max()) and np.abs(r["du"][b] - gu).max() <= 1e-6 * max(1.0, np.abs(gu).max())
    with pytest.raises(RuntimeError):
        emu_step(spec, Z, U, opts=opts, quad=True)


def test_linear_contact_beyond_sixteen_bodies():
    """LinearContact in the lane mapping (an eighteen-link snake with 36 contacts: where the product sends such a mechanism)"""
    spec = d.get_mechanism("snake", num_bodies=18, joint_type="Revolute", contact_type="linear")
    opts = d.SolverOptions(rtol=1e-9, btol=1e-9)
    Z, U = d.synthetic_inputs(spec, 2)
    o = Oracle(spec, opts=opts)
    r = emu_step(spec, Z, U, opts=opts, quad=False)
    for b in range(2):
        zo, info = o.step(Z[b], U[b])
        assert r["status"][b] == 0 and info["status"] == 0 and r["iters"][b] == info["iters"]
        assert np.abs(r["z_next"][b] - zo).max() < 1e-9


@pytest.mark.parametrize("kind", ["spherical", "planar", "cylindrical", "mixed"])
def test_joint_limits_on_several_coordinates(kind):
    """Joint limits on all free coordinates of a half and on both halves of a joint (src/joints/limits.jl:1-61; the -DDJ_MLIM=1 build of the
    lane program, lane mapping): a rollout into the stops against the oracle -- equal Newton iteration counts, states, the exported limit
    variables in get_solution order [s_up(n) s_lo(n) gamma_up(n) gamma_lo(n) lambda] per half, and IFT Jacobians in both conventions."""
    spec = d.get_limited_chain(kind)
    opts = d.SolverOptions(rtol=1e-9, btol=1e-9)
    o = Oracle(spec, opts=opts)
    rng = np.random.default_rng(1)
    z = d.initialize(spec)
    u = 2.0 * rng.standard_normal(spec.nu)
    hit = 0
    for k in range(48):
        zo, info = o.step(z, u)
        if k % 8 == 7 or k < 2:
            mode = (k // 8) % 2
            r = emu_step(spec, z[None], u[None], opts=opts, quad=False, grad=True, grad_mode=mode)
            gz, gu = o.gradients(mode)
            sol = o.get_solution()
            assert r["status"][0] == 0 and info["status"] == 0 and r["iters"][0] == info["iters"], (k, r["iters"][0], info["iters"])
            assert np.abs(r["z_next"][0] - zo).max() < 1e-9
            assert np.abs(r["joint_imp"][0] - sol[:spec.n_joint_impulses]).max() < 1e-8
            assert np.abs(r["dz"][0] - gz).max() <= 1e-6 * max(1.0, np.abs(gz).max()) and np.abs(r["du"][0] - gu).max() <= 1e-6 * max(1.0, np.abs(gu).max())
            hit += int(np.abs(sol[:spec.n_joint_impulses]).max() > 1e-2)
        z = zo
    assert hit >= 2
    with pytest.raises(RuntimeError):
        emu_step(spec, z[None], u[None], opts=opts, quad=True)          # the quad mappings carry one limited coordinate per joint


def test_kinematic_loop_fourbar():
    """A mechanism whose graph is no tree (DojoEnvironments fourbar, test/behaviors.jl:57-81; the reference's LDU handles it through
    `cyclic_children`, src/solver/linear_system.jl:4-5): the loop-closing joint stays out of the tree elimination and comes back through a
    low-rank correction of every solve (LaneProgram::cut_*, the -DDJ_CUT=1 build of the lane program, lane mapping).  Against the oracle (dense
    LU of the whole cyclic system): equal Newton iteration counts, states, every joint's multipliers -- the loop joint's included -- and IFT
    Jacobians in both conventions, with inputs on the loop joint as well."""
    spec = d.get_fourbar(timestep=0.01)
    opts = d.SolverOptions(rtol=1e-9, btol=1e-9)
    o = Oracle(spec, opts=opts)
    rng = np.random.default_rng(0)
    z = d.initialize(spec, inner_angle=0.25)
    for k in range(24):
        u = np.array([rng.random(), -rng.random(), 0.3 * rng.standard_normal(), 0.0, 0.5 * rng.standard_normal()])
        zo, info = o.step(z, u)
        if k % 6 == 0:
            mode = (k // 6) % 2
            r = emu_step(spec, z[None], u[None], opts=opts, quad=False, grad=True, grad_mode=mode)
            gz, gu = o.gradients(mode)
            sol = o.get_solution()
            assert r["status"][0] == 0 and info["status"] == 0 and r["iters"][0] == info["iters"]
            assert np.abs(r["z_next"][0] - zo).max() < 1e-9
            assert np.abs(r["joint_imp"][0] - sol[:spec.n_joint_impulses]).max() < 1e-8
            assert np.abs(r["dz"][0] - gz).max() <= 1e-6 * max(1.0, np.abs(gz).max()) and np.abs(r["du"][0] - gu).max() <= 1e-6 * max(1.0, np.abs(gu).max())
            assert np.abs(gu[:, 4]).max() > 1e-6                        # the loop joint's input does act on the mechanism
        z = zo
    with pytest.raises(RuntimeError):
        emu_step(spec, z[None], u[None], opts=opts, quad=True)



def test_cut_elements_with_several_environments_per_wavefront():
    """the cut elements' workspace is per ENVIRONMENT (KernelArgs::cutws: lane 0 of every environment gathers H and factorizes, every lane of the
    environment reads back): a batch of five environments, four per wavefront (the last wavefront holds one and three empty slots) -- the
    four-bar with gradients and the two free spheres, every environment against the oracle"""
    rng = np.random.default_rng(21)
    spec = d.get_fourbar(timestep=0.01)
    B = 5
    Z = np.stack([d.initialize(spec, inner_angle=0.15 + 0.3 * rng.random(), base_angle=np.pi / 4 + 0.3 * rng.standard_normal()) for _ in range(B)])
    U = rng.standard_normal((B, spec.nu)) * np.array([1.0, 0.3, 1.0, 0.3, 0.5])
    o = Oracle(spec)
    r = emu_step(spec, Z, U, quad=False, grad=True, envs_per_wave=4)
    zo, st_o, it_o, dz_o, du_o = o.step_batch(Z, U, with_grad=True)
    assert np.all(r["status"] == 0) and np.all(st_o == 0) and np.array_equal(r["iters"], it_o)
    assert np.abs(r["z_next"] - zo).max() < 1e-9
    for b in range(B):
        assert np.abs(r["dz"][b] - dz_o[b]).max() <= 1e-6 * max(1.0, np.abs(dz_o[b]).max()) and np.abs(r["du"][b] - du_o[b]).max() <= 1e-6 * max(1.0, np.abs(du_o[b]).max())
    assert np.abs(r["z_next"][0] - r["z_next"][1]).max() > 1e-3                      # (distinct environments)
    spec = d.get_two_spheres(friction_type="nonlinear", gravity=-9.81, joint_world_body1="Floating", free_on="world")
    Z = np.zeros((B, 2, 13)); Z[:, :, 6] = 1.0
    dirs = rng.normal(size=(B, 3)); dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    Z[:, 1, 0:3] = dirs * 1.01; Z[:, 1, 3:6] = -dirs * rng.uniform(0.5, 2.0, size=(B, 1)); Z[:, 1, 10:13] = rng.normal(size=(B, 3))
    Z = Z.reshape(B, -1)
    o = Oracle(spec)
    for k in range(3):
        r = emu_step(spec, Z, np.zeros((B, spec.nu)), quad=False, envs_per_wave=4)
        zo, st_o, it_o = o.step_batch(Z, np.zeros((B, spec.nu)))[:3]
        assert np.array_equal(r["status"], st_o) and np.array_equal(r["iters"], it_o) and np.abs(r["z_next"] - zo).max() < 1e-8
        Z = zo


def ball_on_atlas():
    """Atlas (31 bodies, four contacts per foot) with a ball that hangs in the tree on its upper torso and is thrown at it: a body-body contact
    ALONG A TREE EDGE in a mechanism the tree-edge builds (single-wavefront quad mapping, one contact per body) do not serve"""
    import copy
    from dojo_amd.mechanisms import BodySpec, Floating, sphere_inertia, sphere_sphere_contact
    base = d.baseline_config(5)
    spec = copy.deepcopy(base)
    link = [b.name for b in spec.bodies].index("utorso")
    spec.bodies.append(BodySpec("ball", 2.0, sphere_inertia(0.15, 2.0)))
    spec.joints.append(Floating("ball_free", link, spec.Nb - 1))
    spec.contacts.append(sphere_sphere_contact("ball_on_torso", link, spec.Nb - 1, 0.25, 0.15, 0.6))
    Z0, U0 = d.synthetic_inputs(base, 1)
    zb = np.zeros(13); zb[6] = 1.0
    zb[0:3] = Z0[0][13 * link:13 * link + 3] + np.array([0.03, 0.02, 0.43]); zb[3:6] = Z0[0][13 * link + 3:13 * link + 6] + np.array([0, 0, -1.5])
    return spec, np.concatenate([Z0[0], zb]), np.concatenate([U0[0], np.zeros(6)])


def test_tree_edge_body_body_contacts_outside_the_quad_builds():
    """where the tree-edge builds do not serve a mechanism -- the lane mapping, more than 16 bodies, several contacts per body -- a body-body contact
    between a body and its tree child travels as a cut element (dojo_host.hpp promote_tree_edge_contacts; refused until round 5): the two-sphere
    mechanism through the lane mapping, the ball hanging on the Ant's leg through the lane mapping, and a ball thrown at Atlas's torso (32 bodies,
    nine contacts).  Status and Newton iteration counts equal to the oracle's on every step -- the steps that run into max_iter on both sides
    included --, states to 1e-8 where it converges"""
    for g, joint, x2, v2, w2 in SS_CASES[-2:]:
        spec = d.get_two_spheres(friction_type="nonlinear", gravity=g, joint_world_body1=joint, free_on="body1")
        o = Oracle(spec); z = _two_sphere_state([0, 0, 0], x2, v2, w2)
        for k in range(12):
            zo, info = o.step(z, np.zeros(spec.nu))
            r = emu_step(spec, z[None], np.zeros((1, spec.nu)), quad=False)
            assert r["status"][0] == info["status"] == 0 and r["iters"][0] == info["iters"] and np.abs(r["z_next"][0] - zo).max() < 1e-8, (joint, k)
            z = zo
    for (spec, z, u), steps in ((_ball_on_the_ant(False), 8), (ball_on_atlas(), 5)):
        o = Oracle(spec); loaded = False
        for k in range(steps):
            zo, info = o.step(z, u)
            r = emu_step(spec, z[None], u[None], quad=False)
            assert r["status"][0] == info["status"] and r["iters"][0] == info["iters"], (spec.Nb, k)
            if info["status"] == 0:
                assert np.abs(r["z_next"][0] - zo).max() < 1e-8
            loaded = loaded or o.get_solution()[-4] > 1e-2
            z = zo
        assert loaded


def _both_factorizations(spec, Z, U, steps, envs_per_wave, **kw):
    """the same rollout with the factorization's level passes in the quad layout (DOJO_ROWS=0) and in the row layout (DOJO_ROWS=1)"""
    outs = {}
    old = os.environ.get("DOJO_ROWS")
    try:
        for rows in ("0", "1"):
            os.environ["DOJO_ROWS"] = rows
            z = Z.copy(); seq = []
            for k in range(steps):
                seq.append(emu_step(spec, z, U, quad=True, envs_per_wave=envs_per_wave, grad=(k == steps - 1), **kw))
                z = seq[-1]["z_next"]
            outs[rows] = seq
    finally:
        if old is None: os.environ.pop("DOJO_ROWS", None)
        else: os.environ["DOJO_ROWS"] = old
    return outs["0"], outs["1"]


@pytest.mark.parametrize("cfg", [3, 4])
def test_row_layout_factorization_is_the_quad_one(cfg):
    """LaneProgram::factorize_rows (16 lanes per supernode, the pivot row inside v_fmac_f64_dpp on the GPU) performs the operations of
    factorize_quad in the same order: every output of a rollout -- states, iteration counts, impulses, cone variables, both Jacobians --
    is equal bit for bit.  Ant and Quadruped: one environment per wavefront, level passes of 1 / 4 / 4 / 4 supernodes."""
    spec = d.baseline_config(cfg)
    Z, U = d.synthetic_inputs(spec, 2, seed=11)
    a, b = _both_factorizations(spec, Z, U, steps=3, envs_per_wave=1)
    for ra, rb in zip(a, b):
        assert np.array_equal(ra["iters"], rb["iters"]) and np.array_equal(ra["status"], rb["status"])
        for key in ("z_next", "vel", "joint_imp", "contact_sg", "storage"):
            assert np.array_equal(ra[key], rb[key]), key
    assert np.array_equal(a[-1]["dz"], b[-1]["dz"]) and np.array_equal(a[-1]["du"], b[-1]["du"])
    assert min(r["iters"].min() for r in a) >= 3          # (real solves, not early exits)


def test_row_layout_factorization_over_two_wavefronts():
    """Atlas (31 bodies, two wavefronts per environment, bodies with four contacts): every wavefront runs the row passes of its own sixteen
    supernode slots, both in step, one pass per tree level (11 passes of at most 3 + 3 supernodes); children's Schur complements cross between
    the wavefronts through the mailbox.  Bit for bit against the quad layout."""
    spec = d.baseline_config(5)
    Z, U = d.synthetic_inputs(spec, 1, seed=5, distribution="standing")
    a, b = _both_factorizations(spec, Z, U, steps=2, envs_per_wave=1)
    for ra, rb in zip(a, b):
        assert np.array_equal(ra["iters"], rb["iters"]) and np.array_equal(ra["status"], rb["status"])
        for key in ("z_next", "vel", "joint_imp", "contact_sg"):
            assert np.array_equal(ra[key], rb[key]), key
    assert np.array_equal(a[-1]["dz"], b[-1]["dz"]) and np.array_equal(a[-1]["du"], b[-1]["du"])
    assert min(r["iters"].min() for r in a) >= 3


@pytest.mark.parametrize("seed,nb", [(1, None), (3, 4), (5, 2), (8, 7), (9, 3)])
def test_row_layout_factorization_with_several_environments_per_wavefront(seed, nb):
    """Random trees of 2 .. 8 bodies, 16 / S environments per 64-lane wavefront (S = supernode slots per environment): a level pass of
    the row layout serves supernodes of several environments, levels of more than four supernodes take several passes, and the last
    wavefront of the batch is partly idle (its slots stage identities).  Bit for bit against the quad layout."""
    from random_mechanisms import random_mechanism
    spec, z, u = random_mechanism(seed, nb=nb)
    S = 1
    while S < spec.Nb: S *= 2
    E = 16 // S
    B = E + max(1, E // 2)                                 # one full wavefront and a partly filled one
    rng = np.random.default_rng(seed)
    Z = np.stack([z] * B); U = np.stack([u * (1.0 + 0.3 * rng.normal()) for _ in range(B)])
    opts = d.SolverOptions(rtol=1e-9, btol=1e-9)
    a, b = _both_factorizations(spec, Z, U, steps=2, envs_per_wave=E, opts=opts)
    for ra, rb in zip(a, b):
        assert np.array_equal(ra["iters"], rb["iters"]) and np.array_equal(ra["status"], rb["status"])
        for key in ("z_next", "vel", "joint_imp", "contact_sg"):
            assert np.array_equal(ra[key], rb[key]), key
    assert np.array_equal(a[-1]["dz"], b[-1]["dz"]) and np.array_equal(a[-1]["du"], b[-1]["du"])
    o = Oracle(spec, opts=opts)                            # ... and both are the oracle's step
    zo, info = o.step(Z[0], U[0])
    assert info["iters"] == a[0]["iters"][0] and np.abs(a[0]["z_next"][0] - zo).max() < 1e-10
