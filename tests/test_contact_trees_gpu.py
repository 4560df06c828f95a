"""Every step-kernel build, in both ABI types, on random trees whose contacts are in force (-m gpu): tests/contact_trees.py gives one case or more
per row of g_variants (dojo_hip.hip), `dojo_get_kernel_build` says which row ran, and the CPU oracle -- pinned on these very inputs by
tests/test_contact_trees_references.py -- is what every output is compared with.  The plain / tsd / gen rows with NonlinearContact carry gradients
(test_contact_tree_parity); the lin and ss rows, a body-body contact promoted to a cut element and ImpactContact on the plain rows are forward only
(test_forward_only_contact_tree_parity: the forward outputs, and that no environment's result depends on the batch it ran in).

Bounds (DESIGN.md section 7 has the measured figures per build):
  fp64      state <= 1e-8; dz / du <= 1e-6 relative (|D|inf / max(1, |J|inf)), as test_random_tree_mechanisms_all_mappings; dc <= 1e-6 relative, as
            test_contact_gradient_parity
  fp32 ABI  the oracle gets fp32_abi_state(Z) and rounded controls; state <= 1e-5, gradients <= 1e-3 relative, as test_forward_parity_f32_io and
            test_gradient_parity_f32_io
  contact_sg  [s; gamma] are unknowns of the same solve as the velocities: the bound of the velocities that the state bound implies, state bound / dt
            (1e-6 in fp64, 1e-3 in fp32 at dt = 0.01), relative to max(1, |sg|inf)
Status and iteration counts are equal in every environment and step: the pinned inputs are regular solves of the oracle (<= REGULAR_ITERS), and its dz
moves by <= 1e-7 when its input moves in the last place (reference_spread): what the bounds measure is the kernels."""
import numpy as np
import pytest
import dojo_amd as d
from dojo_amd import api
from contact_trees import CASES, GRADIENT_CASES, FORWARD_RUNS, BUILDS, OPTIONS, contact_tree, reference

pytestmark = pytest.mark.gpu

BOUNDS = {"f64": dict(state=1e-8, grad=1e-6, dc=1e-6, sg=1e-6), "f32": dict(state=1e-5, grad=1e-3, dc=1e-3, sg=1e-3)}


def _rel(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(1.0, np.abs(ref).max())) if ref.size else 0.0


@pytest.mark.parametrize("options", ["default", "tight"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", GRADIENT_CASES)
def test_contact_tree_parity(case, dtype, options):
    """Three steps, each from the oracle's state: status, iterations, next state, exported [s; gamma], dz / du (the step's gradient mode alternates)
    and dc on the quad builds, in every environment; a repeated step and two environments with equal inputs give equal bits."""
    ref = reference(case, dtype, options)
    spec, U, bd = ref["spec"], ref["U"], BOUNDS[dtype]
    B = len(U)
    gm = api.BatchedMechanism(spec, B, dtype=dtype, opts=d.SolverOptions(**OPTIONS[options]))
    build = gm.kernel_build()
    assert build == CASES[case]["build"], build
    worst = dict(state=0.0, sg=0.0, dz=0.0, du=0.0, dc=0.0)
    fails = []
    for k, s in enumerate(ref["steps"]):
        gm.set_gradient_mode(s["mode"])
        Zin, Uin = s["Z"].astype(gm.np_dtype), U.astype(gm.np_dtype)
        zn, st, it = gm.step(Zin, Uin, with_gradient=True)
        dz, du = gm.gradients()
        _, _, sg = gm.get_solution()
        dc = gm.contact_gradients() if build[2] > 0 else None
        print("%s %s %s step %d: status %s / %s iters %s / %s" % (case, dtype, options, k, st, s["status"], it, s["iters"]))
        if not (np.array_equal(st, s["status"]) and np.array_equal(it, s["iters"])):
            fails.append("step %d: status %s / %s, iterations %s / %s" % (k, st, s["status"], it, s["iters"]))
        e = dict(state=float(np.abs(zn.astype(np.float64) - s["Zn"]).max()), sg=_rel(sg, s["csg"]),
                 dz=max(_rel(dz[b], s["dz"][b]) for b in range(B)), du=max(_rel(du[b], s["du"][b]) for b in range(B)) if spec.nu else 0.0,
                 dc=max(_rel(dc[b], s["dc"][b]) for b in range(B)) if dc is not None else 0.0)
        print("    errors / bound: " + "  ".join("%s %.2e / %.0e" % (n, e[n], bd["grad" if n in ("dz", "du") else n]) for n in e))
        for n in e:
            worst[n] = max(worst[n], e[n])
            if not e[n] <= bd["grad" if n in ("dz", "du") else n]:
                fails.append("step %d: %s %.3e > %.0e" % (k, n, e[n], bd["grad" if n in ("dz", "du") else n]))
        # equal inputs at both ends of the batch (the last one sits alone in a ragged workgroup): equal bits
        same = all(np.array_equal(a[0], a[B - 1]) for a in (zn, it, dz, du, sg) + ((dc,) if dc is not None else ()))
        if not same:
            fails.append("step %d: environments 0 and %d have equal inputs and different results" % (k, B - 1))
        if k == 0:                                      # the same step again: bit-identical
            zn2, st2, it2 = gm.step(Zin, Uin, with_gradient=True)
            dz2, du2 = gm.gradients()
            _, _, sg2 = gm.get_solution()
            again = all(np.array_equal(a, b, equal_nan=True) for a, b in ((zn, zn2), (st, st2), (it, it2), (dz, dz2), (du, du2), (sg, sg2)))
            if dc is not None:
                again = again and np.array_equal(dc, gm.contact_gradients(), equal_nan=True)
            if not again:
                fails.append("step 0 repeated: results differ")
    gm.close()
    print("WORST %s %s %s %s %s" % (case, "%s_%d_%d" % build, dtype, options, " ".join("%s=%.2e" % kv for kv in worst.items())))
    assert not fails, fails


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case,options", FORWARD_RUNS)
def test_forward_only_contact_tree_parity(case, options, dtype):
    """Three steps, each from the oracle's state: status, iterations, next state and exported [s; gamma] in every environment; two environments with
    equal inputs and a repeated step give equal bits; a gradient step is refused and leaves the handle as it was; environments 0, 1 and B - 1 stepped
    alone on a handle of batch 1 give the bits they gave in the batch."""
    ref = reference(case, dtype, options, grads=False)
    spec, U, bd = ref["spec"], ref["U"], BOUNDS[dtype]
    B = len(U)
    opts = d.SolverOptions(**OPTIONS[options])
    gm = api.BatchedMechanism(spec, B, dtype=dtype, opts=opts)
    build = gm.kernel_build()
    assert build == CASES[case]["build"], build
    g1 = api.BatchedMechanism(spec, 1, dtype=dtype, opts=opts)
    assert g1.kernel_build() == build

    def forward(h, Z_, U_):
        zn, st, it = h.step(Z_, U_)
        return zn, st, it, h.get_solution()[2]

    worst = dict(state=0.0, sg=0.0)
    fails = []
    for k, s in enumerate(ref["steps"]):
        Zin, Uin = s["Z"].astype(gm.np_dtype), U.astype(gm.np_dtype)
        zn, st, it, sg = out = forward(gm, Zin, Uin)
        print("%s %s %s step %d: status %s / %s iters %s / %s" % (case, dtype, options, k, st, s["status"], it, s["iters"]))
        if not (np.array_equal(st, s["status"]) and np.array_equal(it, s["iters"])):
            fails.append("step %d: status %s / %s, iterations %s / %s" % (k, st, s["status"], it, s["iters"]))
        assert sg.shape == s["csg"].shape
        e = dict(state=float(np.abs(zn.astype(np.float64) - s["Zn"]).max()), sg=_rel(sg, s["csg"]))
        print("    errors / bound: " + "  ".join("%s %.2e / %.0e" % (n, e[n], bd[n]) for n in e))
        for n in e:
            worst[n] = max(worst[n], e[n])
            if not e[n] <= bd[n]:
                fails.append("step %d: %s %.3e > %.0e" % (k, n, e[n], bd[n]))
        if not all(np.array_equal(a[0], a[B - 1]) for a in out):
            fails.append("step %d: environments 0 and %d have equal inputs and different results" % (k, B - 1))
        if k == 0:
            if not all(np.array_equal(a, b, equal_nan=True) for a, b in zip(out, forward(gm, Zin, Uin))):
                fails.append("step 0 repeated: results differ")
            with pytest.raises(api.DojoError, match="error -2"):        # no gradients for these mechanisms: refused, nothing launched ...
                gm.step(Zin, Uin, with_gradient=True)
            if not all(np.array_equal(a, b, equal_nan=True) for a, b in zip(out, forward(gm, Zin, Uin))):
                fails.append("step 0 after the refused gradient step: results differ")      # ... and the handle steps as before
        for b in sorted({0, 1, B - 1}):                                 # alone in a batch of one: the bits of the batch
            if not all(np.array_equal(a[0], c[b], equal_nan=True) for a, c in zip(forward(g1, Zin[b:b + 1], Uin[b:b + 1]), out)):
                fails.append("step %d: environment %d alone differs from the same environment in the batch" % (k, b))
    gm.close(); g1.close()
    print("WORST %s %s %s %s %s" % (case, "%s_%d_%d" % build, dtype, options, " ".join("%s=%.2e" % kv for kv in worst.items())))
    assert not fails, fails


REFUSED = {      # mechanisms no kernel build serves: (case dict for contact_tree, the message's beginning)
    "linear_ball_on_17_bodies": (dict(nb=16, counts="spread", stride=4, balls=1, model="linear"), "a LinearContact body-body contact needs the single-wavefront quad mapping"),
    "linear_ball_next_to_two_contacts_on_one_body": (dict(nb=6, counts=[1, 2, 1], balls=1, ball_on=[1], model="linear"), "a LinearContact body-body contact needs the single-wavefront quad mapping"),
    "three_promoted_balls": (dict(nb=6, counts=[1, 2, 1], balls=3, ball_on=[1, 0, 2]), "more than two cut elements"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_unserved_body_body_contacts_are_refused_at_create(name):
    """dojo_create says DOJO_ERR_UNSUPPORTED and why; no handle, no kernel"""
    case, msg = REFUSED[name]
    spec, Z, U = contact_tree(dict(case, name=name), seed=60, B=3)
    assert spec.Nb == case["nb"] + case["balls"] and sum(k.collision == 1 for k in spec.contacts) == case["balls"]
    for dtype in ("f64", "f32"):
        with pytest.raises(api.DojoError, match="error -2: " + msg):
            api.BatchedMechanism(spec, len(Z), dtype=dtype)


def test_contact_gradients_are_refused_under_the_lane_mapping():
    """dc under the lane mapping: DOJO_ERR_UNSUPPORTED, not columns of some other layout"""
    case = "plain_4_0_nc17"
    spec, Z, U = contact_tree(case)
    gm = api.BatchedMechanism(spec, len(Z), dtype="f64")
    assert gm.kernel_build()[2] == 0
    gm.step(Z, U, with_gradient=True)
    with pytest.raises(api.DojoError, match="error -2"):
        gm.contact_gradients()
    gm.close()


def test_cases_cover_every_build_in_both_abi_types():
    """what dojo_get_kernel_build reports for the cases' mechanisms, together: all 18 rows of g_variants, fp64 and fp32 (36 pairs)"""
    seen = set()
    for case in CASES:
        spec, Z, U = contact_tree(case)
        for dtype in ("f64", "f32"):
            gm = api.BatchedMechanism(spec, len(Z), dtype=dtype)
            seen.add((gm.kernel_build(), dtype)); gm.close()
    want = {(b, t) for b in BUILDS for t in ("f64", "f32")}
    print("COVERED %d (build, type) pairs of %d" % (len(seen & want), len(want)))
    assert len(BUILDS) == 18 and len(want) == 36
    assert seen == want, (sorted(want - seen), sorted(seen - want))
