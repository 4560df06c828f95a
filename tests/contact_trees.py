"""Random trees with contacts in force (test infrastructure): the trees of tests/random_mechanisms.py below a floating root, with contacts of one
model (NonlinearContact, ImpactContact or LinearContact) placed on chosen bodies -- the root, interior bodies that have children, a leaf.  A few of
a case's contacts start on the floor, within a fraction of a millimetre on either side, the others hover centimetres above it (GAP_ON, GAP_OFF below
say why).  One case or more per kernel build (dojo_hip.hip,
g_variants: plain / tsd / gen / lin / ss), at the smallest shapes that reach it; `CASES[name]["build"]` is the build the case is meant for.

A case with `balls` carries free spheres that rest on bodies of the tree through body-body contacts (_add_balls); the cases of the lin and ss rows,
and the ImpactContact cases of the plain rows, are forward only (FORWARD_ONLY: dojo_step refuses their gradients).

The contact's world height h = (x + R(q) origin)_z at the generated state gives radius = h - gap, so the tree does not have to move."""
import numpy as np
import dojo_amd as d
from dojo_amd import coords
from dojo_amd.quat import vrot, qconj
from dojo_amd.mechanisms import BodySpec, Floating, Spherical, add_limits, contact_constraint, sphere_inertia, sphere_sphere_contact, Z_AXIS
from random_mechanisms import random_mechanism

# Gaps to the floor at the generated state.  A few contacts per case start ON the floor, within 0.3 mm of it on either side (deeper inside, and the
# correction throws the tree off the floor for the following steps) -- where a body has two of them, both start inside it, so that the body comes to
# rest on both; the other contacts of the case hover 2 - 5 cm above it: their rows are assembled and solved, their impulses stay at the central path's.
# What the reference's solver takes (rtol = btol = 1e-9, 12 seeds of the 16-body tree with a contact on every body): with the other contacts 1.5 - 4 mm
# above the floor 1 seed of 12 converges for three steps, none in regular solves; with them at 5 cm 9 of 12 converge, 3 in regular solves.
GAP_ON, GAP_OFF = 3e-4, (2e-2, 5e-2)
BODY_FLOOR = 0.4    # the lowest body centre after the tree is lifted (radii stay positive: origins are within 0.2 * sqrt(3) of the centre)

# per case: nb bodies; `counts`: contacts per chosen body in the order [root, interior.., leaf] ("all": one on every body; "spread": one on
# node 0, on the last node and on every `stride`-th body in between); family "plain" | "tsd" | "gen"; build = (family, MAXC, waves) expected of
# dojo_get_kernel_build; vel: scale of the generated velocities (0: the tree is dropped at rest); seed: pinned by
# tests/test_contact_trees_references.py (the oracle alone converges on it in regular solves, with the contacts in force, and its Jacobian is determined there: reference_spread)
CASES = {
    "plain_1_1":        dict(nb=16, counts="all", build=("plain", 1, 1), vel=0.0, seed=63),
    "plain_4_1":        dict(nb=12, counts=[3, 4, 2, 4], build=("plain", 4, 1), vel=0.03, seed=103),
    "plain_8_1":        dict(nb=12, counts=[3, 4, 5, 8], build=("plain", 8, 1), vel=0.0, seed=103),
    "plain_1_2_nb17":   dict(nb=17, counts="spread", stride=2, build=("plain", 1, 2), vel=0.0, seed=79),
    "plain_1_2_nb32":   dict(nb=32, counts="spread", stride=3, build=("plain", 1, 2), vel=0.0, seed=432),
    "plain_4_2":        dict(nb=20, counts=[4, 4, 4, 4], build=("plain", 4, 2), vel=0.0, seed=140),
    "plain_4_0_nc17":   dict(nb=20, counts=[4, 4, 4, 4], extra=1, build=("plain", 4, 0), vel=0.0, seed=140),      # the tree of plain_4_2 plus one contact: out of the two-wavefront pool
    "plain_4_0_nb33":   dict(nb=33, counts=[3, 4, 2, 4], build=("plain", 4, 0), vel=0.03, seed=137),
    "plain_8_0_nb24":   dict(nb=24, counts=[2, 5, 1, 3], build=("plain", 8, 0), vel=0.0, seed=107),
    "plain_8_0_nb33":   dict(nb=33, counts=[2, 8, 1, 3], build=("plain", 8, 0), vel=0.0, seed=61),
    "tsd_1_1":          dict(nb=8, counts="all", family="tsd", build=("tsd", 1, 1), vel=0.0, seed=63),
    "tsd_4_1":          dict(nb=12, counts=[3, 4, 2, 4], family="tsd", build=("tsd", 4, 1), vel=0.03, seed=150),
    "tsd_4_0":          dict(nb=17, counts=[3, 4, 2, 4], family="tsd", build=("tsd", 4, 0), vel=0.0, seed=94),
    "tsd_8_0":          dict(nb=8, counts=[2, 6, 1, 3], family="tsd", build=("tsd", 8, 0), vel=0.0, seed=63),
    "gen_4_0":          dict(nb=8, counts=[3, 4, 2, 4], family="gen", build=("gen", 4, 0), vel=0.0, seed=86),
    "gen_8_0":          dict(nb=8, counts=[2, 7, 1, 3], family="gen", build=("gen", 8, 0), vel=0.0, seed=127),
    # forward only: `model` "impact" | "linear" (ImpactContact / LinearContact on every contact of the case), `balls` free spheres resting on bodies
    # of the tree (_add_balls; `ball_on`: which of the bodies that carry contacts host them), `block`: no tree, _thrown_blocks.  Everything these keys need is drawn from a generator of its own, after the draws above: the sixteen cases above keep
    # their inputs (tests/test_contact_trees_references.py holds a digest of them).  tol8: the pinned seed also meets every condition at rtol = btol = 1e-8.
    "lin_1_1":          dict(nb=8, counts="all", model="linear", build=("lin", 1, 1), vel=0.0, seed=95, tol8=True),
    "lin_4_1":          dict(nb=12, counts=[3, 4, 2, 4], model="linear", build=("lin", 4, 1), vel=0.0, seed=120, tol8=True),
    "lin_4_0":          dict(nb=17, counts=[3, 4, 2, 4], model="linear", build=("lin", 4, 0), vel=0.0, seed=65),
    "lin_8_0":          dict(nb=8, counts=[2, 7, 1, 3], model="linear", build=("lin", 8, 0), vel=0.0, seed=167, tol8=True),
    "lin_8_0_block":    dict(block=True, nb=1, model="linear", build=("lin", 8, 0), seed=252, tol8=True),    # get_block's own 8 corners, thrown at the floor
    "ss_1_1":           dict(nb=6, counts="spread", stride=2, balls=2, build=("ss", 1, 1), vel=0.0, seed=60),
    "ss_1_1_impact":    dict(nb=6, counts="spread", stride=2, balls=2, model="impact", build=("ss", 1, 1), vel=0.0, seed=62, tol8=True),
    "lin_1_1_ss":       dict(nb=6, counts="spread", stride=2, balls=2, model="linear", build=("lin", 1, 1), vel=0.0, seed=162, tol8=True),
    "gen_4_0_promoted": dict(nb=6, counts=[1, 2, 1], balls=1, ball_on=[1], build=("gen", 4, 0), vel=0.0, seed=61),  # the ball's host carries two contacts: no tree-edge build, a cut element
    "impact_1_1":       dict(nb=16, counts="all", model="impact", build=("plain", 1, 1), vel=0.0, seed=60, tol8=True),
    "impact_8_1":       dict(nb=12, counts=[3, 4, 5, 8], model="impact", build=("plain", 8, 1), vel=0.0, seed=66, tol8=True),
    "impact_4_2":       dict(nb=20, counts=[4, 4, 4, 4], model="impact", build=("plain", 4, 2), vel=0.0, seed=61, tol8=True),
    "impact_4_0":       dict(nb=33, counts=[3, 4, 2, 4], model="impact", build=("plain", 4, 0), vel=0.0, seed=61, tol8=True),
}
for _c in CASES.values():
    _c.setdefault("family", "plain"); _c.setdefault("model", "nonlinear"); _c.setdefault("balls", 0)

# every row of g_variants (dojo_hip.hip)
BUILDS = [("plain", 1, 1), ("plain", 4, 1), ("plain", 8, 1), ("plain", 1, 2), ("plain", 4, 2), ("plain", 4, 0), ("plain", 8, 0),
          ("tsd", 1, 1), ("tsd", 4, 1), ("tsd", 4, 0), ("tsd", 8, 0), ("gen", 4, 0), ("gen", 8, 0),
          ("lin", 1, 1), ("lin", 4, 1), ("lin", 4, 0), ("lin", 8, 0), ("ss", 1, 1)]
FORWARD_ONLY = [c for c, v in CASES.items() if v["model"] != "nonlinear" or v["balls"]]      # dojo_step refuses their gradients
GRADIENT_CASES = [c for c in CASES if c not in FORWARD_ONLY]                                 # the sixteen cases of the plain / tsd / gen rows
SG_WIDTH = {"nonlinear": 8, "impact": 8, "linear": 12}      # exported [s; gamma] per contact (LinearContact: six cone pairs)
GAMMA_AT = {"nonlinear": 4, "impact": 4, "linear": 6}       # ... and where the normal impulse gamma stands in it

# A ball: a free sphere on a Floating joint whose parent is a body `a` of the tree, resting on `a` through sphere_sphere_contact(a, ball, R_HOST,
# R_BALL): it starts at x_a + n (R_HOST + R_BALL - g) with n within BALL_TILT of vertical and |g| <= GAP_ON, with the velocity of `a`; gravity keeps
# the contact in force.  The contact's slot belongs to the ball (dojo_host.hpp, build_host_model: the child body owns it), so the host's own
# contacts per body, and with them MAXC, are what the case's `counts` say.
BALL_MASS, R_BALL, R_HOST, BALL_TILT = 0.3, 0.1, 0.15, np.deg2rad(2.0)


def envs_per_workgroup(nb, waves):
    """dojo_hip.hip, geometry_of: supernode slots S = the power of two that holds the bodies; four lanes per slot under the quad mapping"""
    S = 1
    while S < nb:
        S *= 2
    return max(1, 64 * waves // (4 * S) if waves else 64 // S)


def batch_of(case):
    """one environment more than a workgroup holds (the last workgroup is ragged), at least three"""
    c = CASES[case]
    return max(3, envs_per_workgroup(c["nb"] + c["balls"], c["build"][2]) + 1)


def _chosen_bodies(joints, nb, counts, stride, extra):
    """-> [(body, number of contacts, how many of them start on the floor)]: the root, interior bodies that have children, a leaf"""
    children = [[] for _ in range(nb)]
    for j in joints:
        if j.parent >= 0:
            children[j.parent].append(j.child)
    interior = [b for b in range(1, nb) if children[b]]
    leaves = [b for b in range(1, nb) if not children[b]]
    assert children[0] and interior and leaves, "the tree has no interior body"
    if counts in ("all", "spread"):                 # one contact per body: four of them on the floor -- root, two interior bodies, the last body (always a leaf)
        bodies = list(range(nb)) if counts == "all" else [0] + [b for b in range(1, nb - 1) if b % stride == 0 or b == interior[0]][:14] + [nb - 1]
        on = {0, interior[0], nb - 1} | set([b for b in interior[1:] if b in bodies][:1])
        return [(b, 1, int(b in on)) for b in bodies]
    assert len(interior) >= len(counts) - 2, "the tree has too few interior bodies for this case"
    picked = [0] + interior[:len(counts) - 2] + [leaves[-1]]
    out = [(b, n, 2 if i == 1 else 1 if i in (0, len(counts) - 1) else 0) for i, (b, n) in enumerate(zip(picked, counts))]
    if extra:                                       # (one more leaf, after all the others: the contacts before it do not change)
        out.append((leaves[0], extra, 0))
    return out


def contact_tree(case, seed=None, B=None):
    """-> (spec, Z [B, 13 Nb], U [B, nu]): the mechanism of `case` and B perturbed copies of its state (environment B - 1 is a copy of environment 0:
    equal inputs at both ends of the batch)"""
    c = CASES[case] if isinstance(case, str) else dict(dict(family="plain", model="nonlinear", balls=0, vel=0.0, name="adhoc"), **case)   # (a dict: a mechanism
    seed = c["seed"] if seed is None else seed                                                    # outside the case set, with seed and B given)
    B = batch_of(case) if B is None else B
    if c.get("block"):
        return _thrown_blocks(c, seed, B)
    nb, fam = c["nb"], c["family"]
    base, _, _ = random_mechanism(seed, nb=nb, translational=(fam == "tsd"))
    joints = list(base.joints)
    joints[0] = Floating("j0", -1, 0)                                   # a floating root, whatever the tree drew
    rng = np.random.default_rng([seed, nb])                            # (cases of one size and seed share the tree's state and their first contacts)
    if fam == "tsd":                                                    # a spring and a damper on one free translation at least
        tj = [j for j in joints[1:] if j.tra.nl < 3]
        assert tj, "no joint with a free translation in this tree"
        if not any(j.tra.spring != 0 or j.tra.damper != 0 for j in tj):
            tj[0].tra.spring = tj[0].rot.spring = 4.0; tj[0].tra.damper = tj[0].rot.damper = 0.6
    if fam == "gen":
        ks = [k for k in range(1, nb) if joints[k].tra.nl == 3 and joints[k].rot.nl == 0]
        if not ks:                                                      # no Spherical joint in the tree: its first joint becomes one
            j = joints[1]
            joints[1] = Spherical(j.name, j.parent, j.child, j.vertex_parent, j.vertex_child, j.orientation_offset, spring=2.0, damper=0.5)
            ks = [1]
    spec = d.MechanismSpec("%s_%d" % (case if isinstance(case, str) else c["name"], seed), list(base.bodies), joints, [], 0.01, None, -9.81)
    # a state with closed joints from random minimal coordinates (the recipe of random_mechanism, velocities scaled by the case)
    x = np.zeros(2 * spec.nu); o = 0; offs = []
    for j in joints:
        n = j.nu; offs.append(o)
        if n == 6:
            x[o:o + 6] = np.concatenate([[0, 0, 1.0], rng.normal(size=3) * 0.3]); x[o + 6:o + 12] = rng.normal(size=6) * c["vel"]
        elif n > 0:
            x[o:o + n] = rng.uniform(-0.5, 0.5, size=n); x[o + n:o + 2 * n] = rng.normal(size=n) * c["vel"]
        o += 2 * n
    if fam == "gen":                                                    # limits on the three coordinates of the Spherical joint, two of them 2 mrad from the state
        th = x[offs[ks[0]]:offs[ks[0]] + 3]
        add_limits(spec, joints[ks[0]].name, rot_limits=(th - np.array([0.002, 0.3, 0.3]), th + np.array([0.3, 0.002, 0.3])))
    z = coords.minimal_to_maximal(spec, x).reshape(nb, 13)
    z[:, 2] += BODY_FLOOR - z[:, 2].min()                               # (the root floats: lifting the tree keeps every joint closed)
    contacts = []
    for body, n, n_on in _chosen_bodies(joints, nb, c["counts"], c.get("stride", 1), c.get("extra", 0)):
        for i in range(n):
            origin = rng.uniform(-0.2, 0.2, size=3)
            if n_on > 1 and i == n - 1:                                     # the second of a pair: across the body's centre from the first, at its height, so that the body's weight comes down on both
                w = vrot(contacts[-1].origin, z[body, 6:10])
                origin = vrot(np.array([-w[0], -w[1], w[2]]), qconj(z[body, 6:10]))
            h = float((z[body, 0:3] + vrot(origin, z[body, 6:10]))[2])
            g = float(rng.uniform(-1.0, 1.0))
            on = i >= n - n_on                                              # (the body's LAST slots: a build that holds too few of them loses a contact in force)
            gap = (-GAP_ON * (2.0 + g) / 3.0 if n_on > 1 else GAP_ON * g) if on else GAP_OFF[0] + (GAP_OFF[1] - GAP_OFF[0]) * 0.5 * (g + 1.0)
            assert h - gap > 0
            contacts.append(contact_constraint("c%d" % len(contacts), body, Z_AXIS, float(rng.uniform(0.2, 0.9)), origin, h - gap, contact_type=c["model"]))
    spec.contacts.extend(contacts)
    z = z.reshape(-1)
    u0 = rng.normal(size=spec.nu) * 0.3
    Z = np.tile(z, (B, 1)); U = np.tile(u0, (B, 1))
    U[1:B - 1] += rng.normal(size=(max(B - 2, 0), spec.nu)) * 0.2        # controls plus noise ...
    Zv = Z.reshape(B, nb, 13)
    Zv[1:B - 1, :, 3:6] += rng.normal(size=(max(B - 2, 0), nb, 3)) * 0.005      # ... and small velocity noise
    Zv[1:B - 1, :, 10:13] += rng.normal(size=(max(B - 2, 0), nb, 3)) * 0.005
    if c["balls"]:
        Z, U = _add_balls(c, spec, Z, U, np.random.default_rng([seed, nb, c["balls"]]))
    return spec, Z, U


def _add_balls(c, spec, Z, U, rng):
    """appends the case's balls to `spec` (bodies, Floating joints, body-body contacts: after everything the tree has) and their states and zero
    controls to Z and U.  Hosts: `ball_on` counts through the bodies that carry the case's contacts, in their order (default: the root, then the next)"""
    B, nb = len(Z), spec.Nb
    hosts = []
    for k in spec.contacts:
        if k.body not in hosts:
            hosts.append(k.body)
    Zb = [Z.reshape(B, nb, 13)]
    for i, a in enumerate(hosts[h] for h in c.get("ball_on", range(c["balls"]))):
        tilt, az = rng.uniform(0.0, BALL_TILT), rng.uniform(0.0, 2.0 * np.pi)
        n = np.array([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)])
        g = GAP_ON * rng.uniform(-1.0, 1.0)
        ball = spec.Nb
        spec.bodies.append(BodySpec("ball%d" % i, BALL_MASS, sphere_inertia(R_BALL, BALL_MASS)))
        spec.joints.append(Floating("ball%d_free" % i, a, ball))
        spec.contacts.append(sphere_sphere_contact("ball%d_on_%d" % (i, a), a, ball, R_HOST, R_BALL, float(rng.uniform(0.2, 0.9)), c["model"]))
        zb = np.zeros((B, 1, 13)); zb[:, 0, 6] = 1.0
        zb[:, 0, 0:3] = Zb[0][:, a, 0:3] + n * (R_HOST + R_BALL - g)
        zb[:, 0, 3:6] = Zb[0][:, a, 3:6]                                    # (every environment's ball moves with its own host)
        Zb.append(zb)
    Z = np.concatenate(Zb, axis=1).reshape(B, -1)
    U = np.concatenate([U, np.zeros((B, 6 * c["balls"]))], axis=1)
    return Z, U


def _thrown_blocks(c, seed, B):
    """the reference's block with its default 8 corners, thrown at the floor as tests/test_gpu_parity.py (test_linear_contact_parity_and_properties)
    throws it; environment B - 1 is a copy of environment 0"""
    spec = d.get_block(contact_type=c["model"])
    rng = np.random.default_rng([seed, 1])
    Z = np.stack([d.initialize(spec, position=[0, 0, rng.uniform(0.0, 0.2)], velocity=rng.normal(size=3), angular_velocity=rng.normal(size=3) * 0.5)
                  for _ in range(B)])
    Z[B - 1] = Z[0]
    return spec, Z, np.zeros((B, spec.nu))


OPTIONS = {"default": dict(), "tight": dict(rtol=1e-9, btol=1e-9),     # the reference's defaults (the plain kernels) | the refining kernels
           "tol8": dict(rtol=1e-8, btol=1e-8)}      # the tolerance of the LinearContact tests of tests/test_gpu_parity.py: the forward-only cases marked tol8
FORWARD_RUNS = [(c, o) for c in FORWARD_ONLY for o in (("default", "tol8") if CASES[c].get("tol8") else ("default",))]
STEPS = 3
_reference = {}


def reference(case, dtype="f64", options="default", seed=None, grads=True):
    """The oracle's own trajectory of a case, computed once per process and shared (do not modify): STEPS steps of every environment, each from
    the oracle's previous state; step k's Jacobians in gradient mode k % 2.  fp32 ABI: the oracle is given the state the fp32 buffer stands for
    and rounded controls.  The forward-only cases take grads=False.  -> dict(case, spec, U, steps = [dict(Z, Zn, status, iters, csg [B, SG_WIDTH Nc],
    mode, dz, du, dc)])"""
    key = (case, dtype, options, seed, grads)
    if key in _reference:
        return _reference[key]
    from oracle import Oracle
    spec, Z, U = contact_tree(case, seed)
    B = len(Z)
    if dtype == "f32":
        U = U.astype(np.float32).astype(np.float64)
    o = Oracle(spec, opts=d.SolverOptions(**OPTIONS[options]))
    nji, model = spec.n_joint_impulses, CASES[case]["model"]
    assert grads is False or case in GRADIENT_CASES, "the oracle has no Jacobians for this case: pass grads=False"
    want_dc = grads and CASES[case]["build"][2] > 0                     # (the builds that carry the contact-data IFT kernel: the quad mappings)
    steps = []
    for k in range(STEPS):
        Zin = d.fp32_abi_state(Z) if dtype == "f32" else Z.copy()
        s = dict(Z=Zin, Zn=np.zeros_like(Z), status=np.zeros(B, np.int32), iters=np.zeros(B, np.int32),
                 csg=np.zeros((B, SG_WIDTH[model] * len(spec.contacts))), mode=k % 2, dz=[], du=[], dc=[])
        for b in range(B):
            zn, info = o.step(Zin[b], U[b])
            s["Zn"][b] = zn; s["status"][b] = info["status"]; s["iters"][b] = info["iters"]
            s["csg"][b] = exported_sg(o.get_solution()[nji + 6 * spec.Nb:], model)
            if grads and info["status"] == 0:
                gz, gu = o.gradients(mode=k % 2)
                s["dz"].append(gz); s["du"].append(gu)
                s["dc"].append(o.contact_gradients(k % 2) if want_dc else None)
            else:
                s["dz"].append(None); s["du"].append(None); s["dc"].append(None)
        steps.append(s)
        Z = s["Zn"]
    _reference[key] = dict(case=case, spec=spec, U=U, steps=steps)
    return _reference[key]


def exported_sg(tail, model):
    """the oracle's contact unknowns in the layout the device exports: [s(4); gamma(4)] per NonlinearContact and [s(6); gamma(6)] per LinearContact as
    they stand; an ImpactContact's [s, gamma] becomes the device's 8-wide [s, 1, 0, 0, gamma, 1, 0, 0] (friction variables pinned at the neutral vector)"""
    if model != "impact":
        return tail
    out = np.zeros((len(tail) // 2, 8)); out[:, [1, 5]] = 1.0
    out[:, [0, 4]] = tail.reshape(-1, 2)
    return out.reshape(-1)


def in_force(ref, threshold):
    """per step: [B, Nc] bool, the contacts whose normal impulse gamma exceeds `threshold`"""
    model = CASES[ref["case"]]["model"]
    return [s["csg"].reshape(len(s["csg"]), -1, SG_WIDTH[model])[:, :, GAMMA_AT[model]] > threshold for s in ref["steps"]]


def forward_spread(case, options="default", seed=None, trials=2):
    """reference_spread for the forward-only cases, whose only evidence is the forward outputs: -> (largest change of z_next, largest change of
    contact_sg relative to max(1, |sg|inf)) when every entry of the input state moves by up to two units in the last place (inf, inf where status or
    iterations change)"""
    from oracle import Oracle
    ref = reference(case, "f64", options, seed=seed, grads=False)
    spec, model = ref["spec"], CASES[case]["model"]
    o = Oracle(spec, opts=d.SolverOptions(**OPTIONS[options]))
    rng = np.random.default_rng(0)
    wz = wsg = 0.0
    for s in ref["steps"]:
        for b in range(len(s["Z"])):
            for _ in range(trials):
                z = s["Z"][b] * (1.0 + 2.0 ** -52 * rng.integers(-2, 3, size=s["Z"][b].shape))
                zn, info = o.step(z, ref["U"][b])
                if info["status"] != s["status"][b] or info["iters"] != s["iters"][b]:
                    return float("inf"), float("inf")
                sg = exported_sg(o.get_solution()[spec.n_joint_impulses + 6 * spec.Nb:], model)
                wz = max(wz, float(np.abs(zn - s["Zn"][b]).max()))
                wsg = max(wsg, float(np.abs(sg - s["csg"][b]).max() / max(1.0, np.abs(s["csg"][b]).max())))
    return wz, wsg


def reference_spread(case, options="tight", seed=None, trials=2):
    """How well the reference itself is determined on a case: the largest relative change of the oracle's dz (|D|inf / max(1, |J|inf), the norm of the
    GPU tier's bound) when every entry of its input state moves by up to two units in the last place, over all steps and environments (inf where the
    perturbed solve ends otherwise).  A comparison at 1e-6 needs inputs on which this is well below 1e-6: at some states of these trees -- cones at
    gamma / s ~ 1e10 on several bodies of one chain -- it reaches 1e-4, and the oracle cannot say which of two Jacobians 1e-5 apart is right."""
    from oracle import Oracle
    ref = reference(case, "f64", options, seed=seed)
    o = Oracle(ref["spec"], opts=d.SolverOptions(**OPTIONS[options]))
    rng = np.random.default_rng(0)
    worst = 0.0
    for s in ref["steps"]:
        for b in range(len(s["Z"])):
            for _ in range(trials):
                z = s["Z"][b] * (1.0 + 2.0 ** -52 * rng.integers(-2, 3, size=s["Z"][b].shape))
                _, info = o.step(z, ref["U"][b])
                if info["status"] != 0 or info["iters"] != s["iters"][b]:
                    return float("inf")
                gz, _ = o.gradients(mode=s["mode"])
                worst = max(worst, float(np.abs(gz - s["dz"][b]).max() / max(1.0, np.abs(s["dz"][b]).max())))
    return worst


def contacts_per_body(spec):
    n = [0] * spec.Nb
    for k in spec.contacts:
        n[k.body] += 1
    return n


def bodies_with_children(spec):
    return {j.parent for j in spec.joints if j.parent >= 0}
