"""The constrained backward pass on the GPU (include/dojo_hip_constraints.h): dojo_riccati_al_dev against the recursion it implements (tests/al_cases.py, pinned on
the CPU by tests/test_riccati_al_references.py) and against dojo_riccati_box_dev / dojo_riccati_dev, whose bits it must give when no row is live.  Inputs are
synthetic and nothing is stepped: the handles only give the shapes.

Gate per output array: |kernel - ref| <= 32 max(e_ref, 2^-52) max|ref| (+ 2^-23 max|ref| for fp32 handles), riccati_cases.bound, with e_ref the
fp64-against-longdouble distance of the reference on the case (<= 1e-13, asserted on the CPU).  The helpers of tests/test_riccati_gpu.py and
tests/test_riccati_box_gpu.py (handles, guarded outputs, the gate) are used as they are."""
import ctypes as C

import numpy as np
import pytest
import torch

import dojo_amd as d
from dojo_amd import api
from gpu_util import assert_same, dev, guards_intact, tdt_of

import al_cases as AC
import box_cases as BC
import riccati_cases as RC
import test_riccati_box_gpu as RB
import test_riccati_gpu as RG

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -2
FLOATS = RB.FLOATS
PER_STEP = ("K", "kff", "active", "iters")


def teardown_module(module):
    RB.teardown_module(RB)


def launch(gm, H, dev_in, outs, act_off, m):
    """dojo_riccati_al_dev on torch tensors (None = NULL; dev_in also holds U, lo, hi, Cx, Cu, w, y, nc, shared; lim / con False: a NULL struct) -> return code"""
    r = api.DojoRiccati(*[api.addr(dev_in.get(k)) for k in ("A", "Bm", "status", "lx", "lu", "lxx", "luu", "lux", "mu")],
                        *[api.addr(outs.get(k)) for k in ("K", "kff", "fail", "dV", "Vx", "Vxx")], int(act_off), int(m))
    lim = api.DojoControlLimits(api.addr(dev_in.get("lo")), api.addr(dev_in.get("hi")))
    con = api.DojoStageConstraints(*[api.addr(dev_in.get(k)) for k in ("Cx", "Cu", "w", "y")], int(dev_in.get("nc", 0)), int(dev_in.get("shared", 0)))
    return api.lib().dojo_riccati_al_dev(gm.h, int(H), C.byref(r), C.byref(lim) if dev_in.get("lim", True) else None, api.addr(dev_in.get("U")),
                                         C.byref(con) if dev_in.get("con", True) else None, api.addr(outs.get("active")), api.addr(outs.get("iters")), api.torch_stream())


def device_inputs(gm, inp, con, U=None, lo=None, hi=None, mu=None, status=None, shared=False):
    tdt = tdt_of(gm)
    dev_in = {k: dev(v, tdt) for k, v in inp.items()}
    dev_in.update(mu=dev(mu, tdt), status=dev(status, torch.int32), U=dev(U, tdt), lo=dev(lo, tdt), hi=dev(hi, tdt), lim=lo is not None or hi is not None)
    if con is not None:
        dev_in.update({k: dev(con.get(k), tdt) for k in ("Cx", "Cu", "w", "y")}, nc=con["w"].shape[-1], shared=int(shared))
    return dev_in


def run(gm, inp, con, act_off, m, U=None, lo=None, hi=None, mu=None, status=None, shared=False, omit=()):
    """NumPy in -> dict of NumPy outputs (floats as fp64).  con: the dict of al_cases.constraints (Cu may be None; None: nc = 0 with NULL arrays).  Every output
    starts as NaN / -77 between guard elements, which must come back untouched; every element of the integer outputs must have been written"""
    H = inp["A"].shape[0]
    outs = RB.outputs(gm, H, m, omit)
    api._chk(launch(gm, H, device_inputs(gm, inp, con, U, lo, hi, mu, status, shared), outs, act_off, m))
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert guards_intact(t), k
        if k in ("fail", "active", "iters"):
            assert not (t == -77).any(), k
    return {k: t.cpu().numpy().astype(np.float64) if k in FLOATS else t.cpu().numpy() for k, t in outs.items()}


def same(what, a, b):
    assert set(a) == set(b)
    for k in a:
        assert_same((what, k), a[k], b[k])


def errors(r64, rld):
    return {k: float(np.abs(r64[k] - rld[k]).max() / np.abs(rld[k]).max()) for k in RC.OUTPUTS}


# ---------------------------------------------------------------- 1. kernel = recursion ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,H,B", AC.CASES)
def test_kernel_matches_the_reference(shape, H, B, dtype):
    """every accumulator build; one row, a partial block, exactly one block, a full and a partial one, three blocks; rows of every kind.  `shared` gives the bits
    of the same matrices replicated and Cu = NULL those of zeros."""
    name, n, nu, act_off, m = RC.SHAPES[shape]
    f32 = dtype == "f32"
    gm = RG.handle(name, dtype, B)
    inp, con, _, _, _, ref, e, _ = AC.reference(shape, H, B, f32)
    out = run(gm, inp, con, act_off, m)
    assert not out["fail"].any() and not out["active"].any() and not out["iters"].any()
    worst = RG.check(out, ref, e, f32, "%s H=%d B=%d nc=%d %s" % (shape, H, B, AC.NC[shape], dtype))
    print("%s H=%d B=%d nc=%d %s: worst %.2f units" % (shape, H, B, AC.NC[shape], dtype, worst))
    one = dict(con, Cx=np.ascontiguousarray(con["Cx"][0, 0]), Cu=np.ascontiguousarray(con["Cu"][0, 0]))
    a, b = run(gm, inp, one, act_off, m, shared=True), run(gm, inp, AC.replicated(one, H, B), act_off, m)
    same("shared", a, b)
    many = int(AC.live(con["w"], con["y"]).sum()) >= 8 and H > 1              # (enough live rows that the Jacobians certainly matter)
    assert not many or not np.array_equal(a["Vxx"], out["Vxx"])
    a, b = run(gm, inp, dict(con, Cu=None), act_off, m), run(gm, inp, dict(con, Cu=np.zeros_like(con["Cu"])), act_off, m)
    same("Cu NULL", a, b)
    assert not many or not np.array_equal(a["K"], out["K"])
    a, b = run(gm, inp, dict(one, Cu=None), act_off, m, shared=True), run(gm, inp, dict(one, Cu=np.zeros_like(one["Cu"])), act_off, m, shared=True)
    same("shared, Cu NULL", a, b)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,H,B", AC.LIMITED_CASES)
def test_limits_and_constraints_together(shape, H, B, dtype):
    name, n, nu, act_off, m = RC.SHAPES[shape]
    f32 = dtype == "f32"
    gm = RG.handle(name, dtype, B)
    inp, con, U, lo, hi, ref, e, _ = AC.reference(shape, H, B, f32, limited=True)
    out = run(gm, inp, con, act_off, m, U, lo, hi)
    assert not out["fail"].any()
    RG.check(out, ref, e, f32, "limited %s H=%d B=%d %s" % (shape, H, B, dtype))
    assert np.array_equal(out["active"], ref["active"]) and out["active"].any()
    assert not out["K"][RB.bits(out["active"], m)].any()


# ---------------------------------------------------------------- 2. rows that are not loaded ----------------------------------------------------------------
def against_recursion(gm, inp, con, act_off, m, f32, what, **kw):
    out = run(gm, inp, con, act_off, m, **kw)
    r64 = AC.recursion(inp, con, act_off, m, **kw); rld = AC.recursion(inp, con, act_off, m, dtype=np.longdouble, **kw)
    assert np.array_equal(out["fail"], rld["fail"]) and not rld["fail"].any()
    RG.check(out, {k: rld[k].astype(np.float64) for k in RC.OUTPUTS}, errors(r64, rld), f32, what)
    return out


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", ["ant", "atlas"])
def test_dead_rows_and_dead_blocks_are_not_loaded(shape, dtype):
    """NaN in the Jacobians of dead rows changes nothing; a middle block (atlas: rows 16 .. 31) or the first block (ant) entirely dead; terminal-only rows"""
    name, n, nu, act_off, m = RC.SHAPES[shape]
    H, B, f32 = 3, 5, dtype == "f32"
    gm = RG.handle(name, dtype, B)
    inp = RC.inputs(shape, H, B, f32); con = {k: v.copy() for k, v in AC.constraints(shape, H, B, f32).items()}
    con["w"][:, :, 16 if shape == "atlas" else 0:32 if shape == "atlas" else 16] = 0.0; con["y"][:, :, 16 if shape == "atlas" else 0:32 if shape == "atlas" else 16] = 0.0
    dead = ~AC.live(con["w"], con["y"])
    assert dead[:, :, 16 if shape == "atlas" else 0:32 if shape == "atlas" else 16].all() and not dead.all()
    clean = against_recursion(gm, inp, con, act_off, m, f32, "dead block %s %s" % (shape, dtype))
    nan = {k: v.copy() for k, v in con.items()}
    nan["Cx"][dead] = np.nan; nan["Cu"][dead[:H]] = np.nan
    same("NaN in dead rows", run(gm, inp, nan, act_off, m), clean)
    # terminal-only: every row of the stages 0 .. H-1 dead (and NaN), the last stage as it is
    term = {k: v.copy() for k, v in nan.items()}
    term["w"][:H] = 0.0; term["y"][:H] = 0.0; term["Cx"][:H] = np.nan; term["Cu"][:] = np.nan
    out = against_recursion(gm, inp, term, act_off, m, f32, "terminal only %s %s" % (shape, dtype))
    assert not np.array_equal(out["Vxx"], clean["Vxx"])
    plain = RB.run(gm, inp, np.zeros((H, B, nu)), None, None, act_off, m)
    assert not np.array_equal(out["Vxx"], plain["Vxx"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_constraints_at_failed_steps_still_count(dtype):
    """status != 0: A, Bm of that step are NaN and count as zero, its constraint rows are added all the same"""
    name, n, nu, act_off, m = RC.SHAPES["ant"]
    H, B, f32 = 3, 5, dtype == "f32"
    gm = RG.handle(name, dtype, B)
    status = np.zeros((H, B), np.int32); status[2, 0] = 1; status[0, 1] = 2; status[1:3, 2] = -1; status[:, 4] = 3
    inp = {k: v.copy() for k, v in RC.inputs("ant", H, B, f32).items()}
    for k in ("A", "Bm"):
        inp[k][status != 0] = np.nan
    con = AC.constraints("ant", H, B, f32)
    out = against_recursion(gm, inp, con, act_off, m, f32, "failed steps %s" % dtype, status=status)
    none = run(gm, inp, None, act_off, m, status=status)
    assert not np.array_equal(out["K"][:, 4], none["K"][:, 4])                # an environment whose every step failed still sees its rows


# ---------------------------------------------------------------- 3. the bits of the other entries ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,H,B", [("slider", 3, 5), ("cartpole2", 3, 65), ("ant", 3, 5), ("quadruped", 3, 5), ("atlas5", 3, 5), ("atlas", 3, 5)])
def test_no_live_row_gives_the_bits_of_the_box_entry_and_of_the_plain_one(shape, H, B, dtype):
    name, n, nu, act_off, m = RC.SHAPES[shape]
    f32 = dtype == "f32"
    gm = RG.handle(name, dtype, B)
    inp = RC.inputs(shape, H, B, f32); U = BC.controls(shape, H, B, BC.C_MAIN, f32); lo, hi = BC.limits(shape, B, BC.C_MAIN)
    mu = np.linspace(0.0, 1.0, B)
    con = AC.constraints(shape, H, B, f32)
    dead = {"Cx": np.full_like(con["Cx"], np.nan), "Cu": np.full_like(con["Cu"], np.nan), "w": np.zeros_like(con["w"]), "y": np.zeros_like(con["y"])}
    box = RB.run(gm, inp, U, lo, hi, act_off, m, mu=mu)
    assert box["active"].any() and (m == 1 or box["iters"].any())            # the QP runs (m = 1: its only input clamped, nothing is left to iterate on)
    plain = RG.run(gm, inp, act_off, m, mu=mu)
    for what, c in (("nc = 0", None), ("all dead", dead), ("nc = 0, arrays given", AC.constraints(shape, H, B, f32, nc=0))):
        same(what, run(gm, inp, c, act_off, m, U, lo, hi, mu=mu), box)
        for U_ in (None, U):
            out = run(gm, inp, c, act_off, m, U_, None, None, mu=mu)
            for k in plain:
                assert_same((what, "NULL lim", k), out[k], plain[k])
            assert not out["active"].any() and not out["iters"].any()
        inf = np.full((B, m), np.inf)
        out = run(gm, inp, c, act_off, m, U, -inf, inf, mu=mu)
        for k in plain:
            assert_same((what, "infinite", k), out[k], plain[k])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", ["ant", "atlas"])
def test_bit_identical_across_runs_batches_and_places(shape, dtype):
    name, n, nu, act_off, m = RC.SHAPES[shape]
    H, f32, c = 3, dtype == "f32", BC.C_MAIN

    def at(envs):
        B = len(envs)
        lo, hi = BC.limits(shape, B, c)
        return run(RG.handle(name, dtype, B), RC.inputs(shape, H, B, f32, envs=envs), AC.constraints(shape, H, B, f32, envs=envs), act_off, m,
                   BC.controls(shape, H, B, c, f32, envs=envs), lo, hi)

    big = 65 if shape == "ant" else 5
    a, b = at(list(range(big))), at(list(range(big)))
    same("two runs", a, b)
    assert a["active"].any() and not a["fail"].any()
    for envs in ([big - 1, 0, 3, 1, 2], [big - 1], [2]) if big > 5 else ([4, 0, 2, 1, 3], [4], [0]):
        sub = at(envs)
        for i, e in enumerate(envs):
            for k in a:
                x, y = (sub[k][:, i], a[k][:, e]) if k in PER_STEP else (sub[k][i], a[k][e])
                assert_same((k, envs, e), x, y)


# ---------------------------------------------------------------- 4. failures, optional members ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_failure_codes_and_zeros(dtype):
    """environment 1 of 3 carries the defect; the codes and zeros of dojo_riccati_box_dev, the neighbours bit for bit those of the clean run"""
    name, n, nu, act_off, m = RC.SHAPES["ant"]
    H, B, f32, c = 5, 3, dtype == "f32", BC.C_MAIN
    gm = RG.handle(name, dtype, B)
    base = RC.inputs("ant", H, B, f32); con = AC.constraints("ant", H, B, f32); U = BC.controls("ant", H, B, c, f32); lo, hi = BC.limits("ant", B, c)
    clean = run(gm, base, con, act_off, m, U, lo, hi)
    assert not clean["fail"].any()

    def zeros_and_neighbours(out, kbad):
        for k in PER_STEP:
            assert not out[k][:kbad + 1, 1].any(), k
            assert_same(k, out[k][kbad + 1:, 1], clean[k][kbad + 1:, 1])
        assert not out["dV"][1].any() and not out["Vx"][1].any() and not out["Vxx"][1].any()
        for b in (0, 2):
            for k in out:
                assert_same((k, b), RB.env_of(out, k, b), RB.env_of(clean, k, b))

    for kbad in (2, H - 1, 0):
        p = {k: v.copy() for k, v in base.items()}; p["luu"][kbad, 1] = -1.0e4 * np.eye(m)
        out = run(gm, p, con, act_off, m, U, lo, hi)
        assert out["fail"].tolist() == [0, kbad + 1, 0]
        zeros_and_neighbours(out, kbad)
    # a negative weight is not examined: large enough it is a pivot failure of its step
    neg = {k: v.copy() for k, v in con.items()}; neg["w"][3, 1, 0] = -1.0e6; neg["y"][3, 1, 0] = 1.0
    out = run(gm, base, neg, act_off, m, U, lo, hi)
    assert out["fail"].tolist() == [0, 4, 0]
    zeros_and_neighbours(out, 3)
    l = lo.copy(); l[1, 3] = 2.0 * c
    out = run(gm, base, con, act_off, m, U, l, hi)
    assert out["fail"].tolist() == [0, -H, 0]
    zeros_and_neighbours(out, H - 1)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_optional_member_null_in_turn(dtype):
    name, n, nu, act_off, m = RC.SHAPES["cartpole2"]
    H, B, f32, c = 3, 5, dtype == "f32", BC.C_MAIN
    gm = RG.handle(name, dtype, B)
    inp = dict(RC.inputs("cartpole2", H, B, f32)); con = AC.constraints("cartpole2", H, B, f32); U = BC.controls("cartpole2", H, B, c, f32); lo, hi = BC.limits("cartpole2", B, c)
    mu = np.linspace(0.0, 2.0, B); status = np.zeros((H, B), np.int32); status[1, 2] = 1
    kw = dict(mu=mu, status=status)
    full = run(gm, inp, con, act_off, m, U, lo, hi, **kw)
    assert full["active"].any()
    for omit in (("dV",), ("Vx",), ("Vxx",), ("active",), ("iters",), ("dV", "Vx", "Vxx", "active", "iters")):
        out = run(gm, inp, con, act_off, m, U, lo, hi, omit=omit, **kw)
        assert set(out) == set(full) - set(omit)
        for k in out:
            assert_same((omit, k), out[k], full[k])
    inf = np.full((B, m), np.inf)
    for what, a, b in (("lo", (None, hi), (-inf, hi)), ("hi", (lo, None), (lo, inf))):
        x, y = run(gm, inp, con, act_off, m, U, a[0], a[1], **kw), run(gm, inp, con, act_off, m, U, b[0], b[1], **kw)
        same(what, x, y)
        assert not np.array_equal(x["kff"], full["kff"]), what
    x, y = run(gm, dict(inp, lux=None), con, act_off, m, U, lo, hi, **kw), run(gm, dict(inp, lux=np.zeros_like(inp["lux"])), con, act_off, m, U, lo, hi, **kw)
    same("lux", x, y); assert not np.array_equal(x["Vxx"], full["Vxx"])
    x, y = run(gm, inp, con, act_off, m, U, lo, hi, status=status), run(gm, inp, con, act_off, m, U, lo, hi, mu=np.zeros(B), status=status)
    same("mu", x, y); assert not np.array_equal(x["Vxx"], full["Vxx"])
    x, y = run(gm, inp, con, act_off, m, U, lo, hi, mu=mu), run(gm, inp, con, act_off, m, U, lo, hi, mu=mu, status=np.zeros((H, B), np.int32))
    same("status", x, y); assert not np.array_equal(x["Vxx"], full["Vxx"])
    x, y = run(gm, inp, dict(con, Cu=None), act_off, m, U, lo, hi, **kw), run(gm, inp, dict(con, Cu=np.zeros_like(con["Cu"])), act_off, m, U, lo, hi, **kw)
    same("Cu", x, y); assert not np.array_equal(x["Vxx"], full["Vxx"])


# ---------------------------------------------------------------- 5. refusals, the host entry ----------------------------------------------------------------
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
    inp = RC.inputs("cartpole1", H, B); con = AC.constraints("cartpole1", H, B); U = BC.controls("cartpole1", H, B, 0.25); lo, hi = BC.limits("cartpole1", B, 0.25)
    dev_in = device_inputs(gm, inp, con, U, lo, hi)
    outs = RB.outputs(gm, H, m)
    who = "dojo_riccati_al_dev: "
    refused(gm, 0, dev_in, outs, act_off, m, INVALID, who + "H must be >= 1")
    for k in ("A", "Bm", "lx", "lu", "lxx", "luu"):
        refused(gm, H, dict(dev_in, **{k: None}), outs, act_off, m, INVALID, who + "A, Bm, lx, lu, lxx, luu, K, kff and fail must not be NULL")
    for k in ("K", "kff", "fail"):
        refused(gm, H, dev_in, dict(outs, **{k: None}), act_off, m, INVALID, who + "A, Bm, lx, lu, lxx, luu, K, kff and fail must not be NULL")
    for ao, na in ((0, 0), (-1, 1), (1, 2), (2, 1)):
        refused(gm, H, dev_in, outs, ao, na, INVALID, who + "the policy must drive inputs act_off .. act_off + na - 1 inside 0 .. nu - 1")
    refused(gm, H, dict(dev_in, con=False), outs, act_off, m, INVALID, who + "con must not be NULL")
    refused(gm, H, dict(dev_in, nc=-1), outs, act_off, m, INVALID, who + "nc must be >= 0")
    for k in ("Cx", "w", "y"):
        refused(gm, H, dict(dev_in, **{k: None}), outs, act_off, m, INVALID, who + "Cx, w and y must not be NULL with nc > 0")
    refused(gm, H, dict(dev_in, U=None), outs, act_off, m, INVALID, who + "U must not be NULL with limits")
    assert api.lib().dojo_riccati_al_dev(gm.h, H, None, None, None, None, None, None, None) == INVALID and "DojoRiccati record" in gm.last_error()
    # the host entry refuses the same way under its own name, and reads the limits, the weights and the multipliers
    r, c = api.DojoRiccati(), api.DojoStageConstraints()
    assert api.lib().dojo_riccati_al(gm.h, H, C.byref(r), None, None, C.byref(c), None, None) == INVALID and "dojo_riccati_al: A, Bm" in gm.last_error()
    args = (inp["A"], inp["Bm"], inp["lx"], inp["lu"], inp["lxx"], inp["luu"])
    kw = dict(Cu=con["Cu"], U=U, act_off=act_off, na=m)
    bad = lo.copy(); bad[3, 0] = 1.0
    with pytest.raises(api.DojoError, match="dojo_riccati_al: the limits must satisfy lo <= hi and must not be NaN"):
        gm.riccati_al(*args, con["Cx"], con["w"], con["y"], lo=bad, hi=hi, **kw)
    for what, w, y in (("w < 0", -1.0, 0.5), ("NaN w", np.nan, 0.5), ("NaN y", 1.0, np.nan)):
        bw, by = con["w"].copy(), con["y"].copy(); bw[2, 1, 3] = w; by[2, 1, 3] = y
        with pytest.raises(api.DojoError, match="dojo_riccati_al: w must be >= 0 and w, y must not be NaN"):
            gm.riccati_al(*args, con["Cx"], bw, by, **kw)


def test_refuses_mechanisms_without_inputs_with_loops_and_beyond_the_plan():
    def attempt(gm, dummy, m):
        dev_in = {k: dummy for k in ("A", "Bm", "lx", "lu", "lxx", "luu", "U", "lo", "hi", "Cx", "w", "y")}; dev_in["nc"] = 1
        outs = {k: dummy for k in ("K", "kff")}; outs["fail"] = torch.zeros(gm.batch, dtype=torch.int32, device="cuda")
        return launch(gm, 1, dev_in, outs, 0, m)

    for spec, code, text in ((d.get_npendulum(num_bodies=3, base_joint_type="Fixed", rest_joint_type="Fixed"), INVALID, "dojo_riccati_al_dev: the mechanism has no inputs"),
                             (d.get_fourbar(), UNSUPPORTED, "kinematic loop")):
        gm = api.BatchedMechanism(spec, 2, dtype="f64")
        try:
            dummy = torch.zeros(4096, dtype=torch.float64, device="cuda")
            assert attempt(gm, dummy, 1) == code and text in gm.last_error(), gm.last_error()
            assert not dummy.any()
        finally:
            gm.close()
    spec = d.get_nslider(num_bodies=40)                  # n = 80, na = 40: beyond the plan, byte count in the text
    gm = api.BatchedMechanism(spec, 1, dtype="f64")
    try:
        n, m = 2 * spec.nu, spec.nu
        need = 8 * (n * (n + 1) // 2 + max(32 * (n + m), m * n + 2 * m * m) + 2 * n + 4 * m + 8)
        dummy = torch.zeros(80 * 80 * 2, dtype=torch.float64, device="cuda")
        assert attempt(gm, dummy, m) == UNSUPPORTED
        assert "dojo_riccati_al_dev: " in gm.last_error() and "%d bytes of LDS" % need in gm.last_error(), gm.last_error()
        assert not dummy.any()
    finally:
        gm.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_host_entry_equals_the_device_entry(dtype):
    name, n, nu, act_off, m = RC.SHAPES["ant"]
    H, B, f32, c = 3, 5, dtype == "f32", BC.C_MAIN
    gm = RG.handle(name, dtype, B)
    inp = RC.inputs("ant", H, B, f32); con = AC.constraints("ant", H, B, f32); U = BC.controls("ant", H, B, c, f32); lo, hi = BC.limits("ant", B, c)
    mu = np.linspace(0.0, 1.0, B); status = np.zeros((H, B), np.int32); status[1, 3] = 1
    args = (inp["A"], inp["Bm"], inp["lx"], inp["lu"], inp["lxx"], inp["luu"])
    names = ("K", "kff", "dV", "fail", "active", "iters", "Vx", "Vxx")
    ref = run(gm, inp, con, act_off, m, U, lo, hi, mu=mu, status=status)
    got = gm.riccati_al(*args, con["Cx"], con["w"], con["y"], Cu=con["Cu"], U=U, lo=lo, hi=hi, lux=inp["lux"], mu=mu, status=status, act_off=act_off, na=m)
    for k, v in zip(names, got):
        assert np.array_equal(ref[k], v.astype(ref[k].dtype)), k
    assert got[4].any()
    # shared Jacobians, no Cu, no limits, no U
    one = dict(con, Cx=np.ascontiguousarray(con["Cx"][0, 0]), Cu=None)
    ref = run(gm, inp, one, act_off, m, shared=True)
    got = gm.riccati_al(*args, one["Cx"], con["w"], con["y"], shared=True, lux=inp["lux"], act_off=act_off, na=m)
    for k, v in zip(names, got):
        assert np.array_equal(ref[k], v.astype(ref[k].dtype)), k
    out = gm.riccati_al(*args, None, None, None, act_off=act_off, na=m, value=False)                 # nc = 0
    plain = gm.riccati(*args, act_off=act_off, na=m, value=False)
    assert len(out) == 6 and all(np.array_equal(a, b) for a, b in zip(out[:4], plain))
