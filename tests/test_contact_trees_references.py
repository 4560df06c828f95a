"""CPU tier of the contact-tree cases (tests/contact_trees.py): what tests/test_contact_trees_gpu.py compares the kernels with is pinned here with the
reference alone -- the oracle converges on every pinned (case, seed) in regular solves with contacts in force --, the oracle's Jacobians are
checked against central differences of its own step on this ground, and the device program runs two of the cases on the SIMT emulator.

The forward-only cases (LinearContact, ImpactContact, body-body contacts: the lin and ss builds, a promoted cut element, the ImpactContact branch of
the plain builds) are pinned the same way with their own conditions, their reference is shown to be determined in its forward outputs -- all the
evidence they give --, and four of them run on the emulator."""
import copy
import hashlib
import numpy as np
import pytest
import dojo_amd as d
from oracle import Oracle
from contact_trees import (CASES, GRADIENT_CASES, FORWARD_ONLY, FORWARD_RUNS, OPTIONS, STEPS, contact_tree, reference, reference_spread, forward_spread,
                           in_force, bodies_with_children, batch_of)

REGULAR_ITERS = 20          # tests/test_gpu_parity.py: a solve of at most this many Newton iterations follows one iterate path on both sides
IN_FORCE = 1e-4             # a contact whose normal impulse gamma exceeds this touches


def _touching(ref):
    """per step: [B, Nc] contacts in force, and the tangential velocities |s[2:4]| of the exported [s; gamma]"""
    nc = len(ref["spec"].contacts)
    out = []
    for s in ref["steps"]:
        g = s["csg"].reshape(len(s["csg"]), nc, 8)
        out.append((g[:, :, 4] > IN_FORCE, np.linalg.norm(g[:, :, 2:4], axis=2)))
    return out


@pytest.mark.parametrize("options", ["default", "tight"])
@pytest.mark.parametrize("case", GRADIENT_CASES)
def test_pinned_inputs_are_regular_solves_with_contacts_in_force(case, options):
    ref = reference(case, "f64", options, grads=False)
    spec = ref["spec"]
    body = np.array([k.body for k in spec.contacts]); parents = bodies_with_children(spec)
    assert len(ref["U"]) == batch_of(case) >= 3 and len(ref["steps"]) == STEPS
    on_parent = False
    for k, (s, (t, vt)) in enumerate(zip(ref["steps"], _touching(ref))):
        assert (s["status"] == 0).all(), (k, s["status"])
        assert s["iters"].max() <= REGULAR_ITERS, (k, s["iters"])
        assert t.sum(axis=1).max() >= 3, (k, t.sum(axis=1))                   # three contacts in force in one environment, at every step
        on_parent = on_parent or any(t[:, i].any() for i in range(len(body)) if body[i] in parents)
        if CASES[case]["build"][1] >= 4:                                        # two contacts of one body in force at once
            assert any(t[e][body == b].sum() >= 2 for e in range(len(t)) for b in set(body)), k
    assert on_parent                                                            # a contact in force on a body that has children
    # the inputs are what the case says: contacts per body, a floating root, NonlinearContact only
    per_body = np.bincount(body, minlength=spec.Nb)
    maxc, (fam, bmaxc, waves) = per_body.max(), CASES[case]["build"]
    assert maxc <= bmaxc and (bmaxc == 1 or maxc > {4: 1, 8: 4}[bmaxc]) and all(k.model == 0 for k in spec.contacts)
    assert spec.joints[0].parent == -1 and spec.joints[0].nu == 6
    if waves == 2:
        assert len(body) <= 16 and 16 < spec.Nb <= 32
    if case.startswith("plain_1_2"):
        assert per_body[0] == 1 and per_body[-1] == 1


@pytest.mark.parametrize("options", ["default", "tight"])
@pytest.mark.parametrize("case", GRADIENT_CASES)
def test_the_reference_is_determined_on_the_pinned_inputs(case, options):
    """The GPU tier holds the kernels' Jacobians to 1e-6 of the oracle's, so the oracle's must be worth that on every pinned input: moving its input
    state by at most two units in the last place moves its dz by <= 1e-7 (a tenth of the bound).  This is not a formality on these trees: with
    cones at gamma / s ~ 1e10 on several bodies of one chain the same measure reads 1.1e-4 (32 bodies, seed 94, rtol = btol = 1e-9, third step),
    2.3e-6 (20 bodies with 17 contacts, seed 121), 1.2e-6 (the general build's 8-body case, seed 78) -- seeds that pass every other condition of
    this file, and on which both mappings of the device program sit 4.5e-5, 2.4e-6 and 5.5e-7 from the oracle.  Pinned seeds measure <= 1e-9."""
    assert reference_spread(case, options) <= 1e-7


def test_the_cases_hold_sticking_and_sliding_contacts():
    """over the whole set, judged from contact_sg: a contact in force whose tangential velocity is zero, and one that moves"""
    stick = slide = 0
    for case in GRADIENT_CASES:
        for t, vt in _touching(reference(case, "f64", "tight", grads=False)):
            stick += int((t & (vt < 1e-6)).sum()); slide += int((t & (vt > 1e-3)).sum())
        if stick and slide:
            break
    assert stick > 0 and slide > 0, (stick, slide)


def test_seventeen_contacts_are_the_sixteen_of_the_pool_case_plus_one():
    a, _, _ = contact_tree("plain_4_2"); b, _, _ = contact_tree("plain_4_0_nc17")
    assert len(a.contacts) == 16 and len(b.contacts) == 17
    for ka, kb in zip(a.contacts, b.contacts):
        assert ka.body == kb.body and ka.radius == kb.radius and np.array_equal(ka.origin, kb.origin)


def test_oracle_jacobians_are_the_derivatives_of_its_step_on_a_contact_tree():
    """The reference on this ground: dz, du and dc of the oracle (consistent mode) against central differences of the oracle's own step, with a
    contact in force on an interior body.  Differences of step eps = 1e-5 of a solve converged to 1e-9 carry ~1e-9 / eps = 1e-4 of noise and
    eps^2 |J'''| of truncation: the bound is 1e-3 relative to max(1, |J v|)."""
    case = "plain_4_1"
    spec, Z, U = contact_tree(case)
    opts = d.SolverOptions(rtol=1e-9, btol=1e-9)
    o = Oracle(spec, opts=opts)
    z, u = Z[1], U[1]
    zn, info = o.step(z, u)
    assert info["status"] == 0
    nb, nc = spec.Nb, len(spec.contacts)
    g = o.get_solution()[spec.n_joint_impulses + 6 * nb:].reshape(nc, 8)
    parents = bodies_with_children(spec)
    inforce = [i for i, k in enumerate(spec.contacts) if g[i, 4] > IN_FORCE]
    assert any(spec.contacts[i].body in parents and spec.contacts[i].body != 0 for i in inforce)
    dz, du = o.gradients(mode=1)
    dc = o.contact_gradients(1)
    rng = np.random.default_rng(11)
    eps = 1e-5
    rows = [(0, 0), (3, 3), (10, 9)]                       # x, v, omega: (offset in z, offset in the tangent coordinates [x; v; phi; omega])

    def tangent_rows(dzn):
        return np.concatenate([dzn[13 * b + zo:13 * b + zo + 3] for b in range(nb) for zo, _ in rows])

    def pick(v):
        return np.concatenate([v[12 * b + to:12 * b + to + 3] for b in range(nb) for _, to in rows])

    def step_of(orc, z_, u_):
        zz, inf = orc.step(z_, u_)
        assert inf["status"] == 0
        return zz

    for _ in range(3):                                    # state directions (x, v, omega of every body; attitude directions: tests/test_oracle_jacobian.py)
        dirz = np.zeros(13 * nb); tang = np.zeros(12 * nb)
        for b in range(nb):
            for zo, to in rows:
                v = rng.standard_normal(3); dirz[13 * b + zo:13 * b + zo + 3] = v; tang[12 * b + to:12 * b + to + 3] = v
        fd = tangent_rows((step_of(o, z + eps * dirz, u) - step_of(o, z - eps * dirz, u)) / (2 * eps))
        jv = pick(dz @ tang)
        assert np.abs(fd - jv).max() <= 1e-3 * max(1.0, np.abs(jv).max()), ("dz", np.abs(fd - jv).max(), np.abs(jv).max())
        diru = rng.standard_normal(spec.nu)
        fd = tangent_rows((step_of(o, z, u + eps * diru) - step_of(o, z, u - eps * diru)) / (2 * eps))
        jv = pick(du @ diru)
        assert np.abs(fd - jv).max() <= 1e-3 * max(1.0, np.abs(jv).max()), ("du", np.abs(fd - jv).max(), np.abs(jv).max())
    # contact data [friction, radius, origin(3)] of the contacts in force and of one that hovers
    hover = [i for i in range(nc) if i not in inforce][:1]
    for i in inforce + hover:
        for p in range(5):
            zs = []
            for sgn in (1.0, -1.0):
                sp = copy.deepcopy(spec); k = sp.contacts[i]
                if p == 0:
                    k.friction_coefficient += sgn * eps
                elif p == 1:
                    k.radius += sgn * eps
                else:
                    k.origin = k.origin.copy(); k.origin[p - 2] += sgn * eps
                zs.append(step_of(Oracle(sp, opts=opts), z, u))
            fd = tangent_rows((zs[0] - zs[1]) / (2 * eps))
            jv = pick(dc[:, 5 * i + p])
            assert np.abs(fd - jv).max() <= 1e-3 * max(1.0, np.abs(jv).max()), ("dc", i, p, np.abs(fd - jv).max(), np.abs(jv).max())


@pytest.mark.parametrize("quad", [True, False])
@pytest.mark.parametrize("case", ["plain_4_1", "plain_8_1"])
def test_device_program_on_contact_trees_emu(case, quad):
    """The device source on the SIMT emulator, twelve bodies with several contacts per body in force, under both mappings (one step of one
    environment: the emulator runs every lane as a thread): state, iterations, dz, du -- and dc under the quad mapping -- against the oracle, with
    the bounds of the GPU tier's fp64 cases."""
    from emu_wrap import emu_step
    ref = reference(case, "f64", "tight")
    spec, s = ref["spec"], ref["steps"][0]
    b = 1                                                   # the perturbed environment
    out = emu_step(spec, s["Z"][b:b + 1], ref["U"][b:b + 1], opts=d.SolverOptions(**OPTIONS["tight"]), grad=True, grad_mode=s["mode"], quad=quad)
    assert out["status"][0] == s["status"][b] and out["iters"][0] == s["iters"][b]
    rel = lambda a, r: np.abs(a - r).max() / max(1.0, np.abs(r).max())
    e = dict(state=np.abs(out["z_next"][0] - s["Zn"][b]).max(), sg=rel(out["contact_sg"][0], s["csg"][b]), dz=rel(out["dz"][0], s["dz"][b]),
             du=rel(out["du"][0], s["du"][b]), dc=rel(out["dc"][0], s["dc"][b]) if quad else 0.0)
    print(case, "quad" if quad else "lane", " ".join("%s=%.2e" % kv for kv in e.items()))
    assert e["state"] <= 1e-8 and e["sg"] <= 1e-6, e
    assert e["dz"] <= 1e-6 and e["du"] <= 1e-6 and e["dc"] <= 1e-6, e


# sha256 (first 16 hex digits) of Z, U and the contact radii of the sixteen plain / tsd / gen cases, taken before the forward-only cases were added
INPUT_DIGESTS = {
    "plain_1_1": "fbeda6dda791e932", "plain_4_1": "f558cd19ade9a3db", "plain_8_1": "c2a0e0946b3b8a9d", "plain_1_2_nb17": "0ee346234f38b4cc",
    "plain_1_2_nb32": "c7675b6be34eb62a", "plain_4_2": "d7b2cc66e1d140ff", "plain_4_0_nc17": "ec49fa5ac5e86910", "plain_4_0_nb33": "b7ca116d4e47e0d1",
    "plain_8_0_nb24": "b6e5c917ed2627c6", "plain_8_0_nb33": "101a3b3d0b3d3733", "tsd_1_1": "b36da345b0384775", "tsd_4_1": "38867da9a1424ddd",
    "tsd_4_0": "3564e606edb4413c", "tsd_8_0": "66faee9b8a9c87b9", "gen_4_0": "e712dcd8c048baae", "gen_8_0": "30c257aef5a3c314",
}


def test_the_sixteen_gradient_cases_keep_their_inputs():
    """the `model` and `balls` keys draw from a generator of their own: the cases that do not use them produce the inputs they produced before"""
    assert list(INPUT_DIGESTS) == GRADIENT_CASES
    for case, want in INPUT_DIGESTS.items():
        spec, Z, U = contact_tree(case)
        h = hashlib.sha256()
        for a in (Z, U, np.array([k.radius for k in spec.contacts])):
            h.update(np.ascontiguousarray(a, np.float64).tobytes())
        assert h.hexdigest()[:16] == want, case
        assert all(k.model == 0 and k.collision == 0 for k in spec.contacts)


def _half_space(spec):
    """-> ([Nc] bool: a contact with the floor, [Nc] the body whose supernode holds the contact: a body-body contact belongs to its child body)"""
    return (np.array([k.collision == 0 for k in spec.contacts]), np.array([k.child_body if k.collision == 1 else k.body for k in spec.contacts]))


@pytest.mark.parametrize("case,options", FORWARD_RUNS)
def test_forward_only_pinned_inputs_are_regular_solves_with_contacts_in_force(case, options):
    """every environment and step: status 0 in at most REGULAR_ITERS iterations.  Trees: three half-space contacts in force in one environment at
    every step, one of them (at some step) on a body with children; MAXC >= 4: two contacts of one body in force; balls: a body-body contact in force
    in every environment at every step.  The oracle's solves from the fp32 ABI's inputs are regular too (not a formality: the 8-body LinearContact
    tree of seed 78 meets everything else, and at rtol = btol = 1e-8 the oracle runs into max_iter from its fp32-rounded state).  And the inputs are what
    the case says."""
    c = CASES[case]
    ref = reference(case, "f64", options, grads=False)
    spec = ref["spec"]
    hs, owner = _half_space(spec)
    parents = bodies_with_children(spec)
    assert len(ref["U"]) == batch_of(case) >= 3 and len(ref["steps"]) == STEPS
    assert np.array_equal(ref["steps"][0]["Z"][0], ref["steps"][0]["Z"][-1]) and np.array_equal(ref["U"][0], ref["U"][-1])
    on_parent = False
    for k, (s, t) in enumerate(zip(ref["steps"], in_force(ref, IN_FORCE))):
        assert (s["status"] == 0).all(), (k, s["status"])
        assert s["iters"].max() <= REGULAR_ITERS, (k, s["iters"])
        if not c.get("block"):
            assert t[:, hs].sum(axis=1).max() >= 3, (k, t[:, hs].sum(axis=1))
            on_parent = on_parent or any(t[:, i].any() for i in range(len(hs)) if hs[i] and owner[i] in parents)
        if c["build"][1] >= 4:
            assert any((t[e] & hs & (owner == b)).sum() >= 2 for e in range(len(t)) for b in set(owner)), k
        if c["balls"]:
            assert t[:, ~hs].any(axis=1).all(), (k, t[:, ~hs])
    assert on_parent or c.get("block")
    for s in reference(case, "f32", options, grads=False)["steps"]:            # the fp32 ABI's reference (the state an fp32 buffer stands for): regular as well
        assert (s["status"] == 0).all() and s["iters"].max() <= REGULAR_ITERS, (s["status"], s["iters"])
    model = {"nonlinear": 0, "impact": 1, "linear": 2}[c["model"]]
    per_body = np.bincount(owner, minlength=spec.Nb)
    fam, bmaxc, waves = c["build"]
    assert all(k.model == model for k in spec.contacts) and (~hs).sum() == c["balls"] and spec.Nb == c["nb"] + c["balls"]
    assert per_body.max() <= bmaxc and (bmaxc == 1 or per_body.max() > {4: 1, 8: 4}[bmaxc])
    assert (fam == "lin") == (model == 2) and (fam == "ss") == (model != 2 and c["balls"] > 0 and per_body.max() == 1)
    if c["balls"]:                      # every ball hangs on the body it rests on (a tree edge), and on no joint that fixes a distance
        for k in np.array(spec.contacts)[~hs]:
            j = [j for j in spec.joints if j.child == k.child_body]
            assert len(j) == 1 and j[0].parent == k.body and j[0].nu == 6
    if waves == 2:
        assert len(hs) <= 16 and 16 < spec.Nb <= 32
    if waves == 0 and not (fam == "gen"):
        assert spec.Nb > 16 or per_body.max() > 4 or (model != 2 and spec.Nb > 32)


@pytest.mark.parametrize("case,options", FORWARD_RUNS)
def test_the_forward_reference_is_determined_on_the_pinned_inputs(case, options):
    """The forward outputs are all the evidence these cases give, and the GPU tier holds them to 1e-8 (state) and 1e-6 (contact_sg): moving the oracle's
    input state by at most two units in the last place leaves status and iterations alone and moves z_next by <= 1e-9 and contact_sg by <= 1e-7
    relative to max(1, |sg|inf), a tenth of each bound.  (Not a formality either: LinearContact balls, seed 142 at 1e-8, read 1.9e-4 in contact_sg.)"""
    wz, wsg = forward_spread(case, options)
    assert wz <= 1e-9 and wsg <= 1e-7, (wz, wsg)


def test_one_case_holds_two_body_body_contacts_in_force():
    """both balls of one case press on their hosts in one environment at every step"""
    held = []
    for case in FORWARD_ONLY:
        if CASES[case]["balls"] >= 2:
            ref = reference(case, "f64", "default", grads=False)
            hs, _ = _half_space(ref["spec"])
            if all((t[:, ~hs].sum(axis=1) >= 2).any() for t in in_force(ref, IN_FORCE)):
                held.append(case)
    assert held


@pytest.mark.parametrize("case,quad", [("lin_8_0", False), ("ss_1_1", True), ("lin_1_1_ss", True), ("gen_4_0_promoted", False), ("impact_8_1", True)])
def test_device_program_on_forward_only_cases_emu(case, quad):
    """The device source on the SIMT emulator under the mapping the product chooses for the case -- more than four LinearContacts on a body under the
    lane mapping, body-body contacts along tree edges (NonlinearContact and LinearContact) under the quad mapping, a promoted body-body contact as a
    cut element under the lane mapping, ImpactContacts split over the quad on a tree -- one step of the perturbed environment against the oracle with the bounds of the GPU tier's fp64 cases."""
    from emu_wrap import emu_step
    ref = reference(case, "f64", "default", grads=False)
    spec, s = ref["spec"], ref["steps"][0]
    b = 1
    out = emu_step(spec, s["Z"][b:b + 1], ref["U"][b:b + 1], opts=d.SolverOptions(**OPTIONS["default"]), quad=quad)
    assert out["status"][0] == s["status"][b] and out["iters"][0] == s["iters"][b], (out["status"], out["iters"], s["status"][b], s["iters"][b])
    e = dict(state=np.abs(out["z_next"][0] - s["Zn"][b]).max(),
             sg=np.abs(out["contact_sg"][0] - s["csg"][b]).max() / max(1.0, np.abs(s["csg"][b]).max()))
    print(case, "quad" if quad else "lane", " ".join("%s=%.2e" % kv for kv in e.items()))
    assert e["state"] <= 1e-8 and e["sg"] <= 1e-6, e
