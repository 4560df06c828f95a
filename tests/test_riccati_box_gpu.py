"""Control-limited iLQR on the GPU (include/dojo_hip_limits.h): dojo_riccati_box_dev against the recursion it implements (tests/box_cases.py, pinned on the CPU by
tests/test_riccati_box_references.py), dojo_rollout_minimal_box_dev against the clipped law of tests/minimal_cases.py and the stepwise path, and
ilqr.solve_limited on the cartpole.  Inputs of the backward pass are synthetic and nothing is stepped there: the handles only give the shapes.

Gate per output array of the backward pass: |kernel - ref| <= 32 max(e_ref, 2^-52) max|ref| (+ 2^-23 max|ref| for fp32 handles), riccati_cases.bound, with e_ref
the fp64-against-longdouble distance of the reference on the case; the clamped set must equal the reference's exactly (the cases have a strict-complementarity
margin >= 1e-6, asserted on the CPU).  The helpers of tests/test_riccati_gpu.py and tests/test_rollout_minimal_gpu.py (handles, guarded outputs, the stepwise
path) are used as they are."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import dojo_amd as d
from dojo_amd import api, ilqr
from gpu_util import GUARD, assert_same, dev, guards_intact, host, tdt_of

import box_cases as BC
import minimal_cases as MC
import riccati_cases as RC
import test_riccati_gpu as RG
import test_rollout_minimal_gpu as RM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
FLOATS = ("K", "kff", "dV", "Vx", "Vxx")


def teardown_module(module):
    RG.teardown_module(RG); RM.teardown_module(RM)


def guarded_int(shape, tdt):
    """gpu_util.guarded for the integer outputs: -77 between guard elements of 77"""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), 77, dtype=tdt, device="cuda")
    flat[GUARD:GUARD + n] = -77
    return flat[GUARD:GUARD + n].view(tuple(shape))


def outputs(gm, H, m, omit=()):
    outs = RG.outputs(gm, H, m, omit)
    for k, tdt in (("active", torch.int64), ("iters", torch.int32)):
        if k not in omit:
            outs[k] = guarded_int((H, gm.batch), tdt)
    return outs


def launch(gm, H, dev_in, outs, act_off, m):
    """dojo_riccati_box_dev on torch tensors (None = NULL; dev_in also holds U, lo, hi) -> return code"""
    r = api.DojoRiccati(*[api.addr(dev_in.get(k)) for k in ("A", "Bm", "status", "lx", "lu", "lxx", "luu", "lux", "mu")],
                        *[api.addr(outs.get(k)) for k in ("K", "kff", "fail", "dV", "Vx", "Vxx")], int(act_off), int(m))
    lim = api.DojoControlLimits(api.addr(dev_in.get("lo")), api.addr(dev_in.get("hi")))
    return api.lib().dojo_riccati_box_dev(gm.h, int(H), C.byref(r), C.byref(lim) if dev_in.get("lim", True) else None, api.addr(dev_in.get("U")),
                                          api.addr(outs.get("active")), api.addr(outs.get("iters")), api.torch_stream())


def run(gm, inp, U, lo, hi, act_off, m, mu=None, status=None, omit=()):
    """NumPy in -> dict of NumPy outputs (floats as fp64: exact for both ABI types).  Every output starts as NaN / -77 between guard elements, which must come back
    untouched; every element of the integer outputs must have been written (the float ones: the callers look)"""
    H, tdt = inp["A"].shape[0], tdt_of(gm)
    dev_in = {k: dev(v, tdt) for k, v in inp.items()}
    dev_in.update(mu=dev(mu, tdt), status=dev(status, torch.int32), U=dev(U, tdt), lo=dev(lo, tdt), hi=dev(hi, tdt))
    outs = outputs(gm, H, m, omit)
    api._chk(launch(gm, H, dev_in, outs, act_off, m))
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert guards_intact(t), k
        if k in ("fail", "active", "iters"):
            assert not (t == -77).any(), k
    return {k: t.cpu().numpy().astype(np.float64) if k in FLOATS else t.cpu().numpy() for k, t in outs.items()}


def tio(a, f32):
    """fp64 values rounded once to the ABI type, as fp64"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64) if f32 else np.asarray(a, np.float64)


def bits(active, m):
    return (active[..., None] >> np.arange(m)) & 1 != 0


# ---------------------------------------------------------------- 1. kernel = recursion ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("c", BC.CS)
@pytest.mark.parametrize("shape,H,B", BC.GPU_CASES)
def test_kernel_matches_the_reference(shape, H, B, c, dtype):
    """every accumulator build, m = 1, m = nu, more than one workgroup's worth of environments, a horizon over which clamped steps feed later ones, and the largest
    plan.  For fp32 handles the reference sees the inputs rounded to fp32."""
    name, n, nu, act_off, m = RC.SHAPES[shape]
    f32 = dtype == "f32"
    gm = RG.handle(name, dtype, B)
    inp, U, lo, hi, ref, e, _ = BC.reference(shape, H, B, c, f32)
    out = run(gm, inp, U, lo, hi, act_off, m)
    assert not out["fail"].any()
    mask = bits(out["active"], m)
    print("%s H=%d B=%d c=%g %s: clamped share %.2f, qp_iters max %d mean %.2f (reference: max %d)" % (shape, H, B, c, dtype, mask.mean(), out["iters"].max(), out["iters"].mean(), ref["iters"].max()))
    RG.check(out, ref, e, f32, "%s H=%d B=%d c=%g %s" % (shape, H, B, c, dtype))
    assert np.array_equal(out["active"], ref["active"])
    assert not out["K"][mask].any()                                                        # rows of clamped inputs: exactly zero
    u = U[:, :, act_off:act_off + m]
    at_lo = np.abs(ref["kff"] - (lo - u)) <= np.abs(ref["kff"] - (hi - u))
    bound = tio(np.where(at_lo, lo - u, hi - u), f32)                                      # formed in fp64, rounded once
    assert np.array_equal(out["kff"][mask], bound[mask])
    assert (out["iters"] >= 0).all() and not out["iters"][out["active"] == 0].any()
    if c == BC.C_MAIN:
        assert mask.mean() >= 0.25


# ---------------------------------------------------------------- 2. the unconstrained pass's bits ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("c", BC.CS)
@pytest.mark.parametrize("shape,H,B", BC.CASES)
def test_limits_that_clip_nothing_give_the_bits_of_the_unconstrained_pass(shape, H, B, c, dtype):
    name, n, nu, act_off, m = RC.SHAPES[shape]
    f32 = dtype == "f32"
    gm = RG.handle(name, dtype, B)
    inp = RC.inputs(shape, H, B, f32); U = BC.controls(shape, H, B, c, f32)
    mu = np.linspace(0.0, 1.0, B)
    plain = RG.run(gm, inp, act_off, m, mu=mu)
    inf = np.full((B, m), np.inf)
    for what, lo, hi in (("+-inf", -inf, inf), ("NULL", None, None), ("lo only", -inf, None), ("wide", np.full((B, m), -1.0e6), np.full((B, m), 1.0e6))):
        out = run(gm, inp, U, lo, hi, act_off, m, mu=mu)
        for k in plain:
            assert_same((what, k), out[k], plain[k])
        assert not out["active"].any() and not out["iters"].any(), what


# ---------------------------------------------------------------- 3. bit identity ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("c", BC.CS)
@pytest.mark.parametrize("shape", ["ant", "atlas"])
def test_bit_identical_across_runs_batches_and_places(shape, c, dtype):
    name, n, nu, act_off, m = RC.SHAPES[shape]
    H, f32 = 3, dtype == "f32"

    def at(envs):
        B = len(envs)
        lo, hi = BC.limits(shape, B, c)
        return run(RG.handle(name, dtype, B), RC.inputs(shape, H, B, f32, envs=envs), BC.controls(shape, H, B, c, f32, envs=envs), lo, hi, act_off, m)

    big = 65 if shape == "ant" else 5
    a, b = at(list(range(big))), at(list(range(big)))
    for k in a:
        assert_same(("two runs", k), a[k], b[k])
    assert a["active"].any() and a["iters"].any()
    per_step = ("K", "kff", "active", "iters")
    for envs in ([big - 1, 0, 3, 1, 2], [big - 1], [2]) if big > 5 else ([4, 0, 2, 1, 3], [4], [0]):
        sub = at(envs)
        for i, e in enumerate(envs):
            for k in a:
                x, y = (sub[k][:, i], a[k][:, e]) if k in per_step else (sub[k][i], a[k][e])
                assert_same((k, envs, e), x, y)


# ---------------------------------------------------------------- 4. failures ----------------------------------------------------------------
def env_of(out, k, b):
    return out[k][:, b] if k in ("K", "kff", "active", "iters") else out[k][b]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("c", BC.CS)
def test_failure_codes_and_zeros(c, dtype):
    """environment 1 of 3 carries the defect; exact codes, exact zeros, its neighbours bit for bit those of the run without it"""
    name, n, nu, act_off, m = RC.SHAPES["ant"]
    H, B, f32 = 5, 3, dtype == "f32"
    gm = RG.handle(name, dtype, B)
    base = RC.inputs("ant", H, B, f32); U = BC.controls("ant", H, B, c, f32); lo, hi = BC.limits("ant", B, c)
    clean = run(gm, base, U, lo, hi, act_off, m)
    assert not clean["fail"].any()

    def zeros_and_neighbours(out, kbad):
        for k in ("K", "kff", "active", "iters"):
            assert not out[k][:kbad + 1, 1].any(), k
            assert_same(k, out[k][kbad + 1:, 1], clean[k][kbad + 1:, 1])
        assert not out["dV"][1].any() and not out["Vx"][1].any() and not out["Vxx"][1].any()
        for b in (0, 2):
            for k in out:
                assert_same((k, b), env_of(out, k, b), env_of(clean, k, b))

    for kbad in (2, H - 1, 0):           # an indefinite luu, as tests/test_riccati_gpu.py provokes it: in the middle, at the step that starts the sweep, at the one that ends it
        p = {k: v.copy() for k, v in base.items()}; p["luu"][kbad, 1] = -1.0e4 * np.eye(m)
        out = run(gm, p, U, lo, hi, act_off, m)
        assert out["fail"].tolist() == [0, kbad + 1, 0]
        zeros_and_neighbours(out, kbad)
    for what in ("lo > hi", "NaN lo", "NaN hi"):
        l, h = lo.copy(), hi.copy()
        if what == "lo > hi":
            l[1, 3] = 2.0 * c
        elif what == "NaN lo":
            l[1, 0] = np.nan
        else:
            h[1, m - 1] = np.nan
        out = run(gm, base, U, l, h, act_off, m)
        assert out["fail"].tolist() == [0, -H, 0], what
        zeros_and_neighbours(out, H - 1)
    # an empty box at one step only: the limits hold, the control of step 1 does not exist (NaN)
    Ub = U.copy(); Ub[1, 1, act_off + 2] = np.nan
    out = run(gm, base, Ub, lo, hi, act_off, m)
    assert out["fail"].tolist() == [0, -2, 0]
    zeros_and_neighbours(out, 1)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("c", BC.CS)
def test_failed_steps_are_not_read(c, dtype):
    """status != 0: the Jacobians of that step are NaN here and count as zero -- the result is the one of zeros there, bit for bit, and the recursion's"""
    name, n, nu, act_off, m = RC.SHAPES["ant"]
    H, B, f32 = 5, 3, dtype == "f32"
    gm = RG.handle(name, dtype, B)
    status = np.zeros((H, B), np.int32); status[4, 0] = 1; status[0, 1] = 2; status[1:3, 2] = -1
    zeros = {k: v.copy() for k, v in RC.inputs("ant", H, B, f32).items()}; nans = {k: v.copy() for k, v in zeros.items()}
    for k in ("A", "Bm"):
        zeros[k][status != 0] = 0.0; nans[k][status != 0] = np.nan
    U = BC.controls("ant", H, B, c, f32); lo, hi = BC.limits("ant", B, c)
    a, b = run(gm, zeros, U, lo, hi, act_off, m, status=status), run(gm, nans, U, lo, hi, act_off, m, status=status)
    for k in a:
        assert_same(k, a[k], b[k])
    r64 = BC.recursion(nans, U, lo, hi, act_off, m, status=status); rld = BC.recursion(nans, U, lo, hi, act_off, m, status=status, dtype=np.longdouble)
    assert not rld["fail"].any() and np.array_equal(r64["mask"], rld["mask"]) and min(r64["margin"].min(), rld["margin"].min()) >= 1e-6
    e = {k: float(np.abs(r64[k] - rld[k]).max() / np.abs(rld[k]).max()) for k in RC.OUTPUTS}
    RG.check(b, {k: rld[k].astype(np.float64) for k in RC.OUTPUTS}, e, f32, "failed steps c=%g %s" % (c, dtype))
    assert np.array_equal(b["active"], rld["active"]) and not b["fail"].any()


# ---------------------------------------------------------------- 5. optional members ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_optional_member_null_in_turn(dtype):
    name, n, nu, act_off, m = RC.SHAPES["cartpole2"]
    H, B, f32, c = 3, 5, dtype == "f32", BC.C_MAIN
    gm = RG.handle(name, dtype, B)
    inp = dict(RC.inputs("cartpole2", H, B, f32)); U = BC.controls("cartpole2", H, B, c, f32); lo, hi = BC.limits("cartpole2", B, c)
    mu = np.linspace(0.0, 2.0, B); status = np.zeros((H, B), np.int32); status[1, 2] = 1
    full = run(gm, inp, U, lo, hi, act_off, m, mu=mu, status=status)
    assert full["active"].any()
    for omit in (("dV",), ("Vx",), ("Vxx",), ("active",), ("iters",), ("dV", "Vx", "Vxx", "active", "iters")):
        out = run(gm, inp, U, lo, hi, act_off, m, mu=mu, status=status, omit=omit)
        assert set(out) == set(full) - set(omit)
        for k in out:
            assert_same((omit, k), out[k], full[k])
    inf = np.full((B, m), np.inf)
    for what, a, b in (("lo", (None, hi), (-inf, hi)), ("hi", (lo, None), (lo, inf))):
        x, y = run(gm, inp, U, a[0], a[1], act_off, m, mu=mu, status=status), run(gm, inp, U, b[0], b[1], act_off, m, mu=mu, status=status)
        for k in x:
            assert_same((what, k), x[k], y[k])
        assert not np.array_equal(x["kff"], full["kff"]), what                              # ... and the side mattered
    # the optional members of the record, as in the unconstrained pass (that each matters shows in Vxx: a gain row may be clamped to zero either way)
    x, y = run(gm, dict(inp, lux=None), U, lo, hi, act_off, m, mu=mu, status=status), run(gm, dict(inp, lux=np.zeros_like(inp["lux"])), U, lo, hi, act_off, m, mu=mu, status=status)
    assert all(np.array_equal(x[k], y[k]) for k in x) and not np.array_equal(x["Vxx"], full["Vxx"])
    x, y = run(gm, inp, U, lo, hi, act_off, m, status=status), run(gm, inp, U, lo, hi, act_off, m, mu=np.zeros(B), status=status)
    assert all(np.array_equal(x[k], y[k]) for k in x) and not np.array_equal(x["Vxx"], full["Vxx"])
    x, y = run(gm, inp, U, lo, hi, act_off, m, mu=mu), run(gm, inp, U, lo, hi, act_off, m, mu=mu, status=np.zeros((H, B), np.int32))
    assert all(np.array_equal(x[k], y[k]) for k in x) and not np.array_equal(x["Vxx"], full["Vxx"])


# ---------------------------------------------------------------- 6. refusals, the host entry ----------------------------------------------------------------
def refused(gm, H, dev_in, outs, act_off, m, code, text):
    rc = launch(gm, H, dev_in, outs, act_off, m)
    torch.cuda.synchronize()
    assert rc == code, (rc, gm.last_error())
    assert text in gm.last_error(), gm.last_error()
    for k, t in outs.items():
        if t is not None:
            assert guards_intact(t) and bool(torch.isnan(t).all() if k in FLOATS else (t == -77).all()), k       # nothing was launched


def test_refusals_with_their_text():
    name, n, nu, act_off, m = RC.SHAPES["cartpole1"]
    H, B = 3, 5
    gm = RG.handle(name, "f64", B)
    dev_in = {k: dev(v, torch.float64) for k, v in RC.inputs("cartpole1", H, B).items()}
    lo, hi = BC.limits("cartpole1", B, 0.25)
    dev_in.update(U=dev(BC.controls("cartpole1", H, B, 0.25), torch.float64), lo=dev(lo, torch.float64), hi=dev(hi, torch.float64))
    outs = outputs(gm, H, m)
    who = "dojo_riccati_box_dev: "
    refused(gm, 0, dev_in, outs, act_off, m, INVALID, who + "H must be >= 1")
    for k in ("A", "Bm", "lx", "lu", "lxx", "luu"):
        refused(gm, H, dict(dev_in, **{k: None}), outs, act_off, m, INVALID, who + "A, Bm, lx, lu, lxx, luu, K, kff and fail must not be NULL")
    for k in ("K", "kff", "fail"):
        refused(gm, H, dev_in, dict(outs, **{k: None}), act_off, m, INVALID, who + "A, Bm, lx, lu, lxx, luu, K, kff and fail must not be NULL")
    for ao, na in ((0, 0), (-1, 1), (1, 2), (2, 1)):
        refused(gm, H, dev_in, outs, ao, na, INVALID, who + "the policy must drive inputs act_off .. act_off + na - 1 inside 0 .. nu - 1")
    refused(gm, H, dict(dev_in, U=None), outs, act_off, m, INVALID, who + "lim and U must not be NULL")
    refused(gm, H, dict(dev_in, lim=False), outs, act_off, m, INVALID, who + "lim and U must not be NULL")
    assert api.lib().dojo_riccati_box_dev(gm.h, H, None, None, None, None, None, None) == INVALID and "DojoRiccati record" in gm.last_error()
    # the host entry refuses the same way under its own name, and reads the limits
    r, lim = api.DojoRiccati(), api.DojoControlLimits()
    assert api.lib().dojo_riccati_box(gm.h, H, C.byref(r), C.byref(lim), None, None, None) == INVALID and "dojo_riccati_box: A, Bm" in gm.last_error()
    inp = RC.inputs("cartpole1", H, B); U = BC.controls("cartpole1", H, B, 0.25)
    args = (inp["A"], inp["Bm"], inp["lx"], inp["lu"], inp["lxx"], inp["luu"], U)
    bad = lo.copy(); bad[3, 0] = 1.0
    with pytest.raises(api.DojoError, match="dojo_riccati_box: the limits must satisfy lo <= hi and must not be NaN"):
        gm.riccati_box(*args, lo=bad, hi=hi, act_off=act_off, na=m)
    bad = hi.copy(); bad[0, 0] = np.nan
    with pytest.raises(api.DojoError, match="must not be NaN"):
        gm.riccati_box(*args, lo=None, hi=bad, act_off=act_off, na=m)
    with pytest.raises(api.DojoError, match="dojo_rollout_minimal_box: the limits must satisfy lo <= hi"):
        gm.rollout_minimal_box(np.zeros((B, n)), lo=1.0, hi=-1.0, steps=2, act_off=act_off, na=m)


def test_refuses_mechanisms_without_inputs_with_loops_and_beyond_the_plan():
    def attempt(gm, dummy, m):
        dev_in = {k: dummy for k in ("A", "Bm", "lx", "lu", "lxx", "luu", "U", "lo", "hi")}
        outs = {k: dummy for k in ("K", "kff")}; outs["fail"] = torch.zeros(gm.batch, dtype=torch.int32, device="cuda")
        return launch(gm, 1, dev_in, outs, 0, m)

    for spec, code, text in ((d.get_npendulum(num_bodies=3, base_joint_type="Fixed", rest_joint_type="Fixed"), INVALID, "dojo_riccati_box_dev: the mechanism has no inputs"),
                             (d.get_fourbar(), UNSUPPORTED, "kinematic loop")):
        gm = api.BatchedMechanism(spec, 2, dtype="f64")
        try:
            dummy = torch.zeros(4096, dtype=torch.float64, device="cuda")
            assert attempt(gm, dummy, 1) == code and text in gm.last_error(), gm.last_error()
            assert not dummy.any()
        finally:
            gm.close()
    # a chain of 40 sliders: n = 80, na = 40 -> beyond the accumulators and the LDS of the unconstrained plan already: its refusal, byte count in the text
    spec = d.get_nslider(num_bodies=40)
    gm = api.BatchedMechanism(spec, 1, dtype="f64")
    try:
        n, m = 2 * spec.nu, spec.nu
        need = 8 * (n * (n + 1) // 2 + max(32 * (n + m), m * n + 2 * m * m) + 2 * n + 4 * m + 8)
        dummy = torch.zeros(80 * 80 * 2, dtype=torch.float64, device="cuda")
        assert attempt(gm, dummy, m) == UNSUPPORTED
        assert "dojo_riccati_box_dev: " in gm.last_error() and "%d bytes of LDS" % need in gm.last_error(), gm.last_error()
        assert not dummy.any()
    finally:
        gm.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_host_entry_equals_the_device_entry(dtype):
    name, n, nu, act_off, m = RC.SHAPES["ant"]
    H, B, f32, c = 3, 5, dtype == "f32", BC.C_MAIN
    gm = RG.handle(name, dtype, B)
    inp = RC.inputs("ant", H, B, f32); U = BC.controls("ant", H, B, c, f32); lo, hi = BC.limits("ant", B, c)
    mu = np.linspace(0.0, 1.0, B); status = np.zeros((H, B), np.int32); status[1, 3] = 1
    ref = run(gm, inp, U, lo, hi, act_off, m, mu=mu, status=status)
    K, kff, dV, fail, active, iters, Vx, Vxx = gm.riccati_box(inp["A"], inp["Bm"], inp["lx"], inp["lu"], inp["lxx"], inp["luu"], U, lo=lo, hi=hi, lux=inp["lux"], mu=mu,
                                                               status=status, act_off=act_off, na=m)
    for k, v in (("K", K), ("kff", kff), ("dV", dV), ("fail", fail), ("Vx", Vx), ("Vxx", Vxx), ("active", active), ("iters", iters)):
        assert np.array_equal(ref[k], v.astype(ref[k].dtype)), k
    assert active.any()
    out = gm.riccati_box(inp["A"], inp["Bm"], inp["lx"], inp["lu"], inp["lxx"], inp["luu"], U, lo=-c, hi=None, act_off=act_off, na=m, value=False)      # a scalar, a NULL side
    assert len(out) == 6 and not out[3].any() and np.isfinite(out[0]).all()


# ---------------------------------------------------------------- 7. the clamped rollout ----------------------------------------------------------------
def rollout_limits(inp, act_off, m, f32, half=0.05):
    """per environment and input: Ubar of step 0 -+ half, rounded to the ABI type -> lo, hi [B, m]"""
    mid = inp["Ubar"][0][:, act_off:act_off + m]
    return tio(mid - half, f32), tio(mid + half, f32)


def launch_rollout(gm, H, dev_in, outs, act_off, m, lo, hi):
    t = api.DojoTracking(*[api.addr(dev_in.get(k)) for k in RM.INPUTS], *[api.addr(outs.get(k)) for k in RM.OUTPUTS], int(act_off), int(m))
    lim = api.DojoControlLimits(api.addr(lo), api.addr(hi))
    return api.lib().dojo_rollout_minimal_box_dev(gm.h, int(H), C.byref(t), C.byref(lim), api.torch_stream())


def run_rollout(gm, inp, act_off, m, lo, hi, jac=False):
    tdt = tdt_of(gm)
    H = inp["Ubar"].shape[0]
    dev_in = {k: dev(inp.get(k), tdt) for k in RM.INPUTS}
    outs = RM.outputs(gm, H, jac)
    api._chk(launch_rollout(gm, H, dev_in, outs, act_off, m, dev(lo, tdt), dev(hi, tdt)))
    torch.cuda.synchronize()
    res = {}
    for k, t in outs.items():
        assert guards_intact(t), k
        res[k] = t.cpu().numpy()
        assert not (res[k] == -77).any() if k == "status" else not np.isnan(res[k]).any(), k       # every element was written
    return res


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("B", [5, 65])
@pytest.mark.parametrize("shape", ["slider", "cartpole1", "cartpole2", "ant"])
def test_clamped_law_and_dynamics(shape, B, dtype):
    """U_out[k] is the longdouble law at the returned X[k], clipped, within minimal_cases.gate, the driven inputs inside [lo, hi] exactly; X, status (A, Bm on
    cartpole2) are those of the stepwise path at (X[k], U_out[k]) on a second handle, bit for bit; infinite limits: dojo_rollout_minimal_dev's bits"""
    name, n, nu, act_off, m = MC.SHAPES[shape]
    H, f32, jac = 3, dtype == "f32", shape == "cartpole2"
    inp = RM.case(shape, H, B, dtype)
    gm, gm2 = RM.handle(shape, dtype, B), RM.handle(shape, dtype, B, "steps")
    lo, hi = rollout_limits(inp, act_off, m, f32)
    out = run_rollout(gm, inp, act_off, m, lo, hi, jac)
    X, U = out["X"], out["U_out"]
    assert_same("X[0] = x0", X[0], inp["x0"].astype(X.dtype))
    driven = np.zeros(nu, bool); driven[act_off:act_off + m] = True
    Ud = U[:, :, driven].astype(np.float64)
    assert (Ud >= lo).all() and (Ud <= hi).all()
    at_bound = (Ud == lo) | (Ud == hi)
    assert at_bound.any() and not at_bound.all()
    worst = 0.0
    for k in range(H):
        ref, S = MC.law(inp, k, X[k].astype(np.float64), act_off, m, np.longdouble)
        ref[:, driven] = np.clip(ref[:, driven], lo.astype(np.longdouble), hi.astype(np.longdouble))
        err = np.abs(U[k].astype(np.longdouble) - ref).astype(np.float64); lim = MC.gate(ref.astype(np.float64), S, n, f32)
        worst = max(worst, float((err / lim).max()))
        assert (err <= lim).all(), (shape, k, float((err / lim).max()))
        assert_same("undriven inputs", U[k][:, ~driven], inp["Ubar"][k][:, ~driven].astype(U.dtype))
    print("%s B=%d %s: max |U_out - clip(ref)| / gate = %.3f, %.2f of the driven inputs at a bound" % (shape, B, dtype, worst, at_bound.mean()))
    for k in range(H):
        got = RM.steps_on(gm2, X, U, k, jac)
        assert_same(("X", k + 1), X[k + 1], got[0]); assert_same(("status", k), out["status"][k], got[1])
        if jac:
            assert_same(("A", k), out["A"][k], got[2]); assert_same(("Bm", k), out["Bm"][k], got[3])
    plain = RM.run(gm, inp, act_off, m, jac)
    inf = np.full((B, m), np.inf)
    for l, h in ((-inf, inf), (None, None)):
        RM.same_outputs(run_rollout(gm, inp, act_off, m, l, h, jac), plain, "infinite limits")
    assert not np.array_equal(plain["U_out"], U)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rollout_host_entry_and_refusals(dtype):
    shape, H, B = "ant", 3, 5
    name, n, nu, act_off, m = MC.SHAPES[shape]
    gm = RM.handle(shape, dtype, B)
    inp = RM.case(shape, H, B, dtype)
    lo, hi = rollout_limits(inp, act_off, m, dtype == "f32")
    ref = run_rollout(gm, inp, act_off, m, lo, hi, jac=True)
    X, U, st, A, Bm = gm.rollout_minimal_box(inp["x0"], lo=lo, hi=hi, Ubar=inp["Ubar"], Xbar=inp["Xbar"], K=inp["K"], kff=inp["kff"], alpha=inp["alpha"], act_off=act_off, na=m,
                                             jacobians=True)
    RM.same_outputs(ref, {"X": X, "U_out": U, "status": st, "A": A, "Bm": Bm}, "host entry")
    tdt = tdt_of(gm)
    dev_in = {k: dev(inp.get(k), tdt) for k in RM.INPUTS}
    outs = RM.outputs(gm, H)
    t = api.DojoTracking(*[api.addr(dev_in.get(k)) for k in RM.INPUTS], *[api.addr(outs.get(k)) for k in RM.OUTPUTS], act_off, m)
    assert api.lib().dojo_rollout_minimal_box_dev(gm.h, H, C.byref(t), None, api.torch_stream()) == INVALID and "dojo_rollout_minimal_box_dev: lim must not be NULL" in gm.last_error()
    assert launch_rollout(gm, 0, dev_in, outs, act_off, m, None, None) == INVALID and "dojo_rollout_minimal_box_dev: H must be >= 1" in gm.last_error()
    assert launch_rollout(gm, H, dict(dev_in, x0=None), outs, act_off, m, None, None) == INVALID and "dojo_rollout_minimal_box_dev: x0, X and U_out must not be NULL" in gm.last_error()
    torch.cuda.synchronize()
    assert all(guards_intact(v) and bool((v == -77).all() if k == "status" else torch.isnan(v).all()) for k, v in outs.items())


# ---------------------------------------------------------------- 8. control-limited iLQR ----------------------------------------------------------------
DT = torch.float64


def cartpole_problem(B):
    x0 = torch.zeros((B, 4), dtype=DT, device="cuda"); x0[:, 2] = torch.linspace(0.2, np.pi, B, dtype=DT, device="cuda")
    cost = ilqr.QuadraticCost(Q=0.01 * torch.eye(4, dtype=DT, device="cuda"), R=1e-4 * torch.eye(1, dtype=DT, device="cuda"), Qf=10.0 * torch.eye(4, dtype=DT, device="cuda"),
                              x_goal=torch.zeros(4, dtype=DT, device="cuda"))
    return x0, cost


def test_solve_limited_on_the_cartpole():
    """B = 8, H and iters of tests/test_ilqr_gpu.py's cartpole; the limit is half of the largest |u| the unconstrained solve reaches on the same problem"""
    B, H, iters = 8, 30, 6
    gm = api.BatchedMechanism(d.get_cartpole(), B, dtype="f64", opts=d.SolverOptions(rtol=1e-8, btol=1e-8))
    try:
        x0, cost = cartpole_problem(B)
        U0 = torch.zeros((H, B, 2), dtype=DT, device="cuda")
        free = ilqr.solve(gm, x0, U0, cost, iters, act_off=0, na=1)
        F = 0.5 * float(free["U"][:, :, 0].abs().max())
        assert F > 0
        for fused in (False, True):
            res = ilqr.solve_limited(gm, x0, U0, cost, iters, -F, F, act_off=0, na=1, fused=fused)
            torch.cuda.synchronize()
            u = res["U"][:, :, 0].abs()
            print("fused %s: F %.4f, largest |u| %.4f, %d of %d environment-steps at the bound, accepted %s" % (fused, F, float(u.max()), int((u == F).sum()), u.numel(), (res["a"] > 0).sum(1).tolist()))
            assert bool((u <= F).all()) and bool((u == F).any())
            J, a = res["J"].cpu().numpy(), res["a"].cpu().numpy()
            assert J.shape == (iters + 1, B) and np.isfinite(J).all()
            assert (np.diff(J, axis=0)[a > 0] <= 0).all(), J                     # never rises for an environment that accepted
            assert (a > 0).any() and (J[-1] <= J[0]).all()
            assert res["active"].shape == (iters, H, B) and res["active"].dtype == torch.int64 and bool(res["active"].any())
            assert not res["U"][:, :, 1].any()                 # the pole's input is not driven
            assert set(res) == set(free) | {"active"}
        # infinite limits: the bits of solve
        for fused in (False, True):
            ref = free if not fused else ilqr.solve(gm, x0, U0, cost, iters, act_off=0, na=1, fused=True)
            inf = torch.full((1,), float("inf"), dtype=DT, device="cuda")
            res = ilqr.solve_limited(gm, x0, U0, cost, iters, -inf, inf, act_off=0, na=1, fused=fused)
            for k in ref:
                assert torch.equal(ref[k], res[k]), (fused, k)
            assert not res["active"].any()
    finally:
        gm.close()


def test_fused_and_stepwise_limited_forward_passes_agree():
    """forward_pass_fused_box evaluates the law and the clamp in fp64 on the device, forward_pass_box in torch: they agree as tests/test_rollout_minimal_gpu.py has
    forward_pass_fused and forward_pass agree, with controls at the bound in both"""
    B, H = 5, 4
    gm = api.BatchedMechanism(d.get_cartpole(), B, dtype="f64")
    try:
        x0 = torch.zeros((B, 4), dtype=DT, device="cuda"); x0[:, 2] = torch.tensor([0.2, 0.6, 1.5, 2.0, np.pi], dtype=DT, device="cuda")
        U = 0.3 * torch.ones((H, B, 2), dtype=DT, device="cuda")
        X, A, Bm, status = ilqr.linearize_rollout(gm, x0, U)
        K = 0.1 * torch.ones((H, B, 1, 4), dtype=DT, device="cuda"); kff = 0.2 * torch.ones((H, B, 1), dtype=DT, device="cuda")
        lo, hi = torch.tensor([0.25], dtype=DT, device="cuda"), torch.tensor([0.35], dtype=DT, device="cuda")
        Xs, Us, ss = ilqr.forward_pass_box(gm, X, U, K, kff, 0.5, 0, 1, lo, hi)
        Xf, Uf, sf = ilqr.forward_pass_fused_box(gm, X, U, K, kff, 0.5, 0, 1, lo, hi)
        assert torch.equal(ss, sf)
        assert float((Xs - Xf).abs().max()) < 1e-9 and float((Us - Uf).abs().max()) < 1e-12
        assert bool((Uf[:, :, 0] == 0.35).any()) and bool((Uf[:, :, 0] <= 0.35).all()) and bool((Uf[:, :, 0] >= 0.25).all())
        assert torch.equal((Us[:, :, 0] == 0.35), (Uf[:, :, 0] == 0.35))
    finally:
        gm.close()


def test_example_runs_with_a_limit_at_a_small_batch():
    spec = importlib.util.spec_from_file_location("cartpole_ilqr_device", os.path.join(ROOT, "examples", "cartpole_ilqr_device.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    res = mod.main(["3", "20", "3", "--limit", "2.0"])
    J = res["J"].cpu().numpy()
    assert J.shape == (4, 3) and (J[-1] <= J[0]).all()
    assert float(res["U"][:, :, 0].abs().max()) <= 2.0 and "active" in res
