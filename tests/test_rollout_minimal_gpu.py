"""Rollouts in minimal coordinates with the tracking controller on the GPU (dojo_rollout_minimal_dev, include/dojo_hip_trajopt.h) against the stepwise path they
replace -- dojo_step_minimal_dev / dojo_minimal_gradients_dev at the recorded (X[k], U_out[k]) on a SECOND handle with the same options, bit for bit -- and against
the control law of tests/minimal_cases.py in longdouble, recomputed from the returned X[k]:

    |U_out - ref| <= (n + 4) 2^-53 S + 1/2 ulp_TIO(|ref|),   S = |Ubar| + |alpha kff| + sum_j |K_ij| |dx_j|     (minimal_cases.gate; derived, not tuned)

Every output is a gpu_util.guarded buffer whose guards must come back intact; every element must have been written."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import dojo_amd as d
from dojo_amd import api, ilqr
from gpu_util import assert_same, dev, guarded, guards_intact, host, tdt_of

import minimal_cases as MC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
INPUTS, OUTPUTS = ("x0", "Ubar", "Xbar", "K", "kff", "alpha"), ("X", "U_out", "status", "A", "Bm")
_handles, _cases = {}, {}


def handle(shape, dtype, B, tag="fused"):
    """one handle per (mechanism, dtype, batch, role) for the whole module; "fused" runs the new entry, "steps" the stepwise path"""
    key = (MC.SHAPES[shape][0], dtype, B, tag)
    if key not in _handles:
        _handles[key] = api.BatchedMechanism(MC.spec_of(shape), B, dtype=dtype)
    return _handles[key]


def teardown_module(module):
    for gm in _handles.values():
        gm.close()
    _handles.clear(); _cases.clear()


def case(shape, H, B, dtype, envs=None):
    """the inputs of a case with Xbar = the open-loop trajectory of Ubar from the perturbed start, stepped by ilqr.replay on the stepwise handle: computed once, shared"""
    key = (shape, H, B, dtype, None if envs is None else tuple(envs))
    if key not in _cases:
        f32 = dtype == "f32"
        gm2 = handle(shape, dtype, B, "steps")
        inp = MC.with_reference(MC.inputs(shape, H, B, f32, envs), lambda x, U: host(ilqr.replay(gm2, dev(x, tdt_of(gm2)), dev(U, tdt_of(gm2)))), f32)
        for v in inp.values():
            v.setflags(write=False)
        _cases[key] = inp
    return _cases[key]


def outputs(gm, H, jac=False, omit=()):
    B, nu, tdt = gm.batch, gm.spec.nu, tdt_of(gm); n = 2 * nu
    shapes = {"X": (H + 1, B, n), "U_out": (H, B, nu), "status": (H, B)}
    if jac:
        shapes.update(A=(H, B, n, n), Bm=(H, B, n, nu))
    return {k: guarded(s, torch.int32 if k == "status" else tdt) for k, s in shapes.items() if k not in omit}


def launch(gm, H, dev_in, outs, act_off, m):
    t = api.DojoTracking(*[api.addr(dev_in.get(k)) for k in INPUTS], *[api.addr(outs.get(k)) for k in OUTPUTS], int(act_off), int(m))
    return api.lib().dojo_rollout_minimal_dev(gm.h, int(H), C.byref(t), api.torch_stream())


def run(gm, inp, act_off, m, jac=False, omit=()):
    """NumPy in (members of inp that are None or missing = NULL) -> dict of NumPy outputs in the handle dtype"""
    tdt = tdt_of(gm)
    H = next(inp[k] for k in ("Ubar", "K", "kff") if inp.get(k) is not None).shape[0]
    dev_in = {k: dev(inp.get(k), tdt) for k in INPUTS}
    outs = outputs(gm, H, jac, omit)
    api._chk(launch(gm, H, dev_in, outs, act_off, m))
    torch.cuda.synchronize()
    res = {}
    for k, t in outs.items():
        assert guards_intact(t), k
        res[k] = t.cpu().numpy()
        assert not (res[k] == -77).any() if k == "status" else not np.isnan(res[k]).any(), k       # every element was written
    return res


def same_outputs(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert_same((what, k), a[k], b[k])


def steps_on(gm2, X, U, k, jac=False):
    """step k of the stepwise path at (X[k], U[k]) on the second handle -> x_next, status (and jx, ju), NumPy"""
    tdt = tdt_of(gm2); B, nu = gm2.batch, gm2.spec.nu; n = 2 * nu
    x, u = dev(X[k], tdt), dev(U[k], tdt)
    xn = guarded((B, n), tdt); st = guarded((B,), torch.int32); it = torch.empty(B, dtype=torch.int32, device="cuda")
    L, s = api.lib(), api.torch_stream()
    if not jac:
        api._chk(L.dojo_step_minimal_dev(gm2.h, api.addr(x), api.addr(u), api.addr(xn), api.addr(st), api.addr(it), s))
        return host(xn), host(st)
    jx = guarded((B, n, n), tdt); ju = guarded((B, n, nu), tdt)
    api._chk(L.dojo_minimal_gradients_dev(gm2.h, api.addr(x), api.addr(u), api.addr(xn), api.addr(st), api.addr(it), api.addr(jx), api.addr(ju), s))
    return host(xn), host(st), host(jx), host(ju)


# ---------------------------------------------------------------- 1. the control law and the dynamics ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,H,B", MC.CASES)
def test_law_and_dynamics(shape, H, B, dtype):
    """U_out[k] is the longdouble law at the returned X[k] within the gate, the inputs that are not driven are Ubar's bits; X[k + 1], status[k] are those of
    dojo_step_minimal_dev(X[k], U_out[k]) on a second handle, bit for bit, all environments counted"""
    name, n, nu, act_off, m = MC.SHAPES[shape]
    f32 = dtype == "f32"
    inp = case(shape, H, B, dtype)
    out = run(handle(shape, dtype, B), inp, act_off, m)
    X, U = out["X"], out["U_out"]
    assert_same("X[0] = x0", X[0], inp["x0"].astype(X.dtype))
    driven = np.zeros(nu, bool); driven[act_off:act_off + m] = True
    worst = 0.0
    for k in range(H):
        ref, S = MC.law(inp, k, X[k].astype(np.float64), act_off, m, np.longdouble)
        err = np.abs(U[k].astype(np.longdouble) - ref).astype(np.float64); lim = MC.gate(ref.astype(np.float64), S, n, f32)
        worst = max(worst, float((err / lim).max()))
        assert (err <= lim).all(), (shape, k, float((err / lim).max()))
        assert_same("undriven inputs", U[k][:, ~driven], inp["Ubar"][k][:, ~driven].astype(U.dtype))
    print("%s H=%d B=%d %s: max |U_out - ref| / gate = %.3f" % (shape, H, B, dtype, worst))
    gm2 = handle(shape, dtype, B, "steps")
    moved = False
    for k in range(H):
        xn, st = steps_on(gm2, X, U, k)
        assert_same(("X", k + 1), X[k + 1], xn); assert_same(("status", k), out["status"][k], st)
        moved |= bool((X[k + 1] != X[k]).any())
    assert moved and np.isfinite(X[:, out["status"].max(0) == 0]).all()
    # the feedback did something: the controls differ from the reference's
    assert (U[:, :, driven] != inp["Ubar"][:, :, driven].astype(U.dtype)).any()


def test_bits_of_the_stepwise_path_over_many_environment_steps():
    """Ant fp32, B = 2048, H = 20 (half of tools/ilqr_forward_bench.py's workload, several environment groups): X, A, Bm, status of the one call are those of the
    H calls of dojo_minimal_gradients_dev, bit for bit.  The small cases cannot see what this one does: a controller kernel with the two coordinate maps fused into
    it passed all of them and differed in the last bit on 68 of the benchmark's 81 920 environment-steps (other multiply-add contractions in rarely taken branches
    of the joint maps) -- one in 1200, so 40 960 environment-steps see it."""
    B, H = 2048, 20
    spec = MC.spec_of("ant")
    gm = api.BatchedMechanism(spec, B, dtype="f32")
    try:
        z0, u = d.synthetic_inputs(spec, B)
        rng = np.random.default_rng(1)
        x0 = dev(gm.maximal_to_minimal(z0.astype(np.float32)), torch.float32)
        U = dev(np.stack([u * rng.uniform(0.5, 1.0) for _ in range(H)]), torch.float32)
        a, b = ilqr.linearize_rollout(gm, x0, U), ilqr.linearize_rollout_fused(gm, x0, U)
        torch.cuda.synchronize()
        Xg, _, sg = ilqr.rollout_minimal(gm, x0, U, na=1)             # without A, Bm: the same states, the batch in several groups on their own streams
        torch.cuda.synchronize()
        for x, y, k in zip(a, b, ("X", "A", "Bm", "status")):
            assert_same(k, y.cpu().numpy(), x.cpu().numpy())
        assert_same("X, groups", Xg.cpu().numpy(), a[0].cpu().numpy()); assert_same("status, groups", sg.cpu().numpy(), a[3].cpu().numpy())
        assert int((a[3] == 0).sum()) > 0.99 * H * B
    finally:
        gm.close()


# ---------------------------------------------------------------- 2. the Jacobians ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mode", [api.GRAD_CONSISTENT, api.GRAD_REFERENCE])
@pytest.mark.parametrize("shape,B", [("slider", 5), ("cartpole1", 5), ("ant", 5), ("ant", 65)])
def test_jacobians_are_those_of_minimal_gradients(shape, B, mode, dtype):
    name, n, nu, act_off, m = MC.SHAPES[shape]
    H = 3
    inp = case(shape, H, B, dtype)
    gm, gm2 = handle(shape, dtype, B), handle(shape, dtype, B, "steps")
    try:
        gm.set_gradient_mode(mode); gm2.set_gradient_mode(mode)
        plain = run(gm, inp, act_off, m)
        out = run(gm, inp, act_off, m, jac=True)
        for k in ("X", "U_out", "status"):
            assert_same(("with and without A, Bm", k), out[k], plain[k])
        for k in range(H):
            xn, st, jx, ju = steps_on(gm2, out["X"], out["U_out"], k, jac=True)
            assert_same(("X", k + 1), out["X"][k + 1], xn); assert_same(("status", k), out["status"][k], st)
            assert_same(("A", k), out["A"][k], jx); assert_same(("Bm", k), out["Bm"][k], ju)
        assert np.isfinite(out["A"]).all() and out["A"].any() and out["Bm"].any()
    finally:
        gm.set_gradient_mode(api.GRAD_REFERENCE); gm2.set_gradient_mode(api.GRAD_REFERENCE)


# ---------------------------------------------------------------- 3. determinism ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", ["cartpole1", "ant"])
def test_bit_identical_across_runs_groups_and_batches(shape, dtype):
    name, n, nu, act_off, m = MC.SHAPES[shape]
    H = 3
    gm = handle(shape, dtype, 65)
    inp = case(shape, H, 65, dtype)
    a = run(gm, inp, act_off, m, jac=True)
    same_outputs(a, run(gm, inp, act_off, m, jac=True), "two runs")
    # one group against several: 65 environments with dojo_set_groups(3) (a group may end inside a workgroup of the controller), and 130 = groups of 128 and 2.
    # With A, Bm the rollout is one group whatever is set (the chain's scratch: one queue's worth); without them the groups apply, so both are run
    for jac in (True, False):
        plain = a if jac else {k: a[k] for k in ("X", "U_out", "status")}
        try:
            gm.set_groups(3); three = run(gm, inp, act_off, m, jac=jac)
            gm.set_groups(1); one = run(gm, inp, act_off, m, jac=jac)
        finally:
            gm.set_groups(0)
        same_outputs(plain, three, "3 groups"); same_outputs(plain, one, "1 group")
        if shape == "ant":
            gm130 = handle(shape, dtype, 130); inp130 = dict(MC.inputs(shape, H, 130, dtype == "f32"), Xbar=None)
            try:
                gm130.set_groups(3); three = run(gm130, inp130, act_off, m, jac=jac)
                gm130.set_groups(1); one = run(gm130, inp130, act_off, m, jac=jac)
            finally:
                gm130.set_groups(0)
            same_outputs(one, three, "130 environments, 1 group against several")
    # the shared leading environments of B = 1 / 5 / 65 (Xbar is stepped per batch by the stepwise path: the big batch's rows are given to the small ones)
    for B in (1, 5):
        sub = dict(MC.inputs(shape, H, B, dtype == "f32"), Xbar=inp["Xbar"][:, :B])
        s = run(handle(shape, dtype, B), sub, act_off, m, jac=True)
        for k in s:
            assert_same(("B = %d" % B, k), s[k], a[k][:, :B])


# ---------------------------------------------------------------- 4. optional members ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_optional_member_null_in_turn(dtype):
    shape, H, B = "cartpole1", 3, 5
    name, n, nu, act_off, m = MC.SHAPES[shape]
    gm = handle(shape, dtype, B)
    inp = dict(case(shape, H, B, dtype))
    full = run(gm, inp, act_off, m, jac=True)
    defaults = {"Ubar": np.zeros((H, B, nu)), "Xbar": np.zeros((H + 1, B, n)), "K": np.zeros((H, B, m, n)), "kff": np.zeros((H, B, m)), "alpha": np.ones(B)}
    for k, dflt in defaults.items():
        a, b = run(gm, dict(inp, **{k: None}), act_off, m, jac=True), run(gm, dict(inp, **{k: dflt}), act_off, m, jac=True)
        same_outputs(a, b, "%s = NULL" % k)
        assert not np.array_equal(a["U_out"], full["U_out"]), k              # ... and the member mattered
    # outputs: status, A + Bm
    a = run(gm, inp, act_off, m, jac=True, omit=("status",))
    assert set(a) == set(full) - {"status"}
    for k in a:
        assert_same(("status = NULL", k), a[k], full[k])
    a = run(gm, inp, act_off, m)
    for k in a:
        assert_same(("A = Bm = NULL", k), a[k], full[k])
    # K = NULL, kff = NULL: the open loop of ilqr.replay
    tdt = tdt_of(gm)
    a = run(gm, dict(inp, K=None, kff=None), act_off, m)
    assert_same("open loop", a["X"], host(ilqr.replay(handle(shape, dtype, B, "steps"), dev(inp["x0"], tdt), dev(inp["Ubar"], tdt))))
    assert_same("open loop", a["U_out"], inp["Ubar"].astype(a["U_out"].dtype))


# ---------------------------------------------------------------- 5. the host entry ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_host_entry_equals_the_device_entry(dtype):
    shape, H, B = "ant", 3, 5
    name, n, nu, act_off, m = MC.SHAPES[shape]
    gm = handle(shape, dtype, B)
    inp = case(shape, H, B, dtype)
    ref = run(gm, inp, act_off, m, jac=True)
    X, U, st, A, Bm = gm.rollout_minimal(inp["x0"], Ubar=inp["Ubar"], Xbar=inp["Xbar"], K=inp["K"], kff=inp["kff"], alpha=inp["alpha"], act_off=act_off, na=m, jacobians=True)
    same_outputs(ref, {"X": X, "U_out": U, "status": st, "A": A, "Bm": Bm}, "host entry")
    X, U, st = gm.rollout_minimal(inp["x0"], steps=H, act_off=act_off, na=m)                 # every optional member NULL: the passive rollout
    assert X.shape == (H + 1, B, n) and not U.any() and np.isfinite(X).all()


# ---------------------------------------------------------------- 6. refusals ----------------------------------------------------------------
def refused(gm, H, dev_in, outs, act_off, m, code, text):
    rc = launch(gm, H, dev_in, outs, act_off, m)
    torch.cuda.synchronize()
    assert rc == code, (rc, gm.last_error())
    assert text in gm.last_error(), gm.last_error()
    for k, t in outs.items():
        if t is not None:
            assert guards_intact(t) and bool((t == -77).all() if k == "status" else torch.isnan(t).all()), k       # nothing was launched


def test_refusals_with_their_text():
    shape, H, B = "cartpole1", 3, 5
    name, n, nu, act_off, m = MC.SHAPES[shape]
    gm = handle(shape, "f64", B)
    dev_in = {k: dev(v, torch.float64) for k, v in case(shape, H, B, "f64").items() if k in INPUTS}
    outs = outputs(gm, H, jac=True)
    who = "dojo_rollout_minimal_dev: "
    refused(gm, 0, dev_in, outs, act_off, m, INVALID, who + "H must be >= 1")
    refused(gm, H, dict(dev_in, x0=None), outs, act_off, m, INVALID, who + "x0, X and U_out must not be NULL")
    for k in ("X", "U_out"):
        refused(gm, H, dev_in, dict(outs, **{k: None}), act_off, m, INVALID, who + "x0, X and U_out must not be NULL")
    for ao, na in ((0, 0), (-1, 1), (1, 2), (2, 1)):
        refused(gm, H, dev_in, outs, ao, na, INVALID, who + "the controller must drive inputs act_off .. act_off + na - 1 inside 0 .. nu - 1")
    for k in ("A", "Bm"):
        refused(gm, H, dev_in, dict(outs, **{k: None}), act_off, m, INVALID, who + "A and Bm must both be given or both be NULL")
    assert api.lib().dojo_rollout_minimal_dev(gm.h, H, None, None) == INVALID and "DojoTracking record" in gm.last_error()
    # the host entry refuses the same way, under its own name
    t = api.DojoTracking()
    assert api.lib().dojo_rollout_minimal(gm.h, H, C.byref(t)) == INVALID and "dojo_rollout_minimal: x0, X and U_out" in gm.last_error()
    with pytest.raises(api.DojoError, match="H must be >= 1"):
        gm.rollout_minimal(np.zeros((B, n)), steps=0)


def test_refuses_mechanisms_without_inputs_with_loops_and_without_gradients():
    """(the controller keeps nothing in LDS: there is no refusal for the size of a shape)"""
    for spec, jac, code, text in ((d.get_npendulum(num_bodies=3, base_joint_type="Fixed", rest_joint_type="Fixed"), False, INVALID, "no inputs"),
                                  (d.get_fourbar(), False, UNSUPPORTED, "kinematic loop"),
                                  (d.get_sphere(contact_type="linear"), True, UNSUPPORTED, "dojo_rollout_minimal_dev: gradients are not available for ImpactContact / LinearContact")):
        gm = api.BatchedMechanism(spec, 2, dtype="f64")
        try:
            dummy = torch.zeros(4096, dtype=torch.float64, device="cuda")
            outs = {"X": dummy, "U_out": dummy, "status": torch.zeros(64, dtype=torch.int32, device="cuda"), "A": dummy if jac else None, "Bm": dummy if jac else None}
            assert launch(gm, 1, {"x0": dummy, "Ubar": dummy}, outs, 0, 1) == code and text in gm.last_error(), gm.last_error()
            torch.cuda.synchronize()
            assert not dummy.any() and not outs["status"].any()
        finally:
            gm.close()


# ---------------------------------------------------------------- 7. iLQR on the fused rollouts ----------------------------------------------------------------
DT = torch.float64


def t64(a):
    return torch.tensor(a, dtype=DT, device="cuda")


def test_fused_rollouts_equal_the_stepwise_ones_in_ilqr():
    """linearize_rollout_fused = linearize_rollout bit for bit; forward_pass_fused evaluates the law in fp64 on the device, forward_pass in torch: its controls are
    the longdouble law's within the gate, and its states those of the stepwise path at its own controls (test 1) -- here: close to forward_pass's"""
    B, H = 5, 4
    gm = api.BatchedMechanism(d.get_cartpole(), B, dtype="f64")
    try:
        x0 = torch.zeros((B, 4), dtype=DT, device="cuda"); x0[:, 2] = t64([0.2, 0.6, 1.5, 2.0, np.pi])
        U = 0.3 * torch.ones((H, B, 2), dtype=DT, device="cuda")
        a, b = ilqr.linearize_rollout(gm, x0, U), ilqr.linearize_rollout_fused(gm, x0, U)
        for x, y, k in zip(a, b, ("X", "A", "Bm", "status")):
            assert torch.equal(x, y), k
        K = 0.1 * torch.ones((H, B, 1, 4), dtype=DT, device="cuda"); kff = 0.2 * torch.ones((H, B, 1), dtype=DT, device="cuda")
        Xs, Us, ss = ilqr.forward_pass(gm, a[0], U, K, kff, 0.5, 0, 1)
        Xf, Uf, sf = ilqr.forward_pass_fused(gm, a[0], U, K, kff, 0.5, 0, 1)
        Xt, Ut, _ = ilqr.forward_pass_fused(gm, a[0], U, K, kff, torch.full((B,), 0.5, dtype=DT, device="cuda"), 0, 1)
        assert torch.equal(Xf, Xt) and torch.equal(Uf, Ut) and torch.equal(ss, sf)
        assert float((Xs - Xf).abs().max()) < 1e-9 and float((Us - Uf).abs().max()) < 1e-12
    finally:
        gm.close()


def test_slider_is_solved_by_one_fused_iteration():
    """tests/test_ilqr_gpu.py's slider test with fused=True, under its gates"""
    B, H = 3, 10
    gm = api.BatchedMechanism(d.get_mechanism("slider"), B, dtype="f64", opts=d.SolverOptions(rtol=1e-10, btol=1e-10))
    try:
        x0 = t64([[0.0, 0.0], [0.3, -0.5], [-0.2, 1.0]])
        U0 = torch.zeros((H, B, 1), dtype=DT, device="cuda")
        cost = ilqr.QuadraticCost(Q=torch.eye(2, dtype=DT, device="cuda"), R=0.1 * torch.eye(1, dtype=DT, device="cuda"), Qf=10.0 * torch.eye(2, dtype=DT, device="cuda"),
                                  x_goal=t64([0.5, 0.0]))
        res = ilqr.solve(gm, x0, U0, cost, 2, fused=True)
        torch.cuda.synchronize()
        assert not res["fail"].any()
        assert (res["a"][0] == 1.0).all(), res["a"]
        dV = res["dV"].cpu().numpy()
        first, second = np.abs(dV[0].sum(-1)), np.abs(dV[1].sum(-1))
        assert (first > 0).all() and (second <= 1e-6 * first).all(), (first, second)
        J = res["J"].cpu().numpy()
        assert (J[1] < J[0]).all() and (np.abs(J[2] - J[1]) <= 1e-6 * np.abs(J[0] - J[1])).all()
        assert np.allclose(J[1] - J[0], dV[0].sum(-1), rtol=1e-6)
    finally:
        gm.close()


def test_cartpole_costs_fall_per_environment_fused():
    """the cartpole case of tests/test_ilqr_gpu.py with fused=True: costs never rise, end below the start, no fail"""
    B, H, iters = 4, 30, 6
    gm = api.BatchedMechanism(d.get_cartpole(), B, dtype="f64", opts=d.SolverOptions(rtol=1e-8, btol=1e-8))
    try:
        x0 = torch.zeros((B, 4), dtype=DT, device="cuda"); x0[:, 2] = t64([0.2, 0.6, 1.5, np.pi])
        U0 = torch.zeros((H, B, 2), dtype=DT, device="cuda")
        cost = ilqr.QuadraticCost(Q=0.01 * torch.eye(4, dtype=DT, device="cuda"), R=1e-4 * torch.eye(1, dtype=DT, device="cuda"), Qf=10.0 * torch.eye(4, dtype=DT, device="cuda"),
                                  x_goal=torch.zeros(4, dtype=DT, device="cuda"))
        res = ilqr.solve(gm, x0, U0, cost, iters, act_off=0, na=1, fused=True)
        torch.cuda.synchronize()
        J = res["J"].cpu().numpy()
        assert J.shape == (iters + 1, B) and np.isfinite(J).all()
        assert (np.diff(J, axis=0) <= 0).all(), J
        assert (J[-1] < J[0]).all(), J
        assert not res["fail"][-1].any()
        assert not res["U"][:, :, 1].any()                 # the pole's input is not driven
    finally:
        gm.close()


def test_example_runs_fused_at_a_small_batch():
    spec = importlib.util.spec_from_file_location("cartpole_ilqr_device", os.path.join(ROOT, "examples", "cartpole_ilqr_device.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    res = mod.main(["3", "20", "3", "--fused"])
    J = res["J"].cpu().numpy()
    assert J.shape == (4, 3) and (J[-1] < J[0]).all()
