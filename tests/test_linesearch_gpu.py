"""The side-by-side line search on the GPU (include/dojo_hip_linesearch.h).

The selection kernel dojo_linesearch_select_dev against the NumPy reference of tests/linesearch_cases.py (longdouble) on synthetic trials: `choice` and `alpha_acc`
exact, the gathers bit copies, the costs (double whatever the handle dtype) within 32 max(e_ref, 2^-52) max|ref|.  The cases keep every trial at least
1e-9 max(1, |J0|) from its threshold (tests/test_linesearch_references.py), so rounding cannot flip a decision.

The fan rollout dojo_rollout_minimal_fan_dev against dojo_rollout_minimal_box_dev (without limits: dojo_rollout_minimal_dev) on the same handle with every
reference member repeated T times: X, U_out, status bit for bit.

The driver ilqr.solve_side_by_side against ilqr.solve_limited(fused=True).

Every output is a gpu_util.guarded buffer whose guards must come back intact; every element must have been written."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dojo_amd as d
from dojo_amd import api, ilqr
from gpu_util import assert_same, dev, guarded, guards_intact, tdt_of

import linesearch_cases as LC
import minimal_cases as MC
import test_riccati_box_gpu as RB
import test_rollout_minimal_gpu as RM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
LS_IN = ("X", "U", "status", "alpha", "dV", "ok", "Xcur", "Ucur", "J0")
LS_OUT = ("J_trial", "J_cur", "J_acc", "choice", "alpha_acc", "X_new", "U_new")
IDS = ["%s-H%d-T%d-P%d" % c for c in LC.CASES]


def teardown_module(module):
    RB.teardown_module(RB)


def handle(shape, dtype, B):
    return RM.handle(shape, dtype, B, "linesearch")


# ================================================================ the selection kernel ================================================================
def select_buffers(gm, H, T, inp, supplied=None, omit=()):
    """device inputs (int32 arrays as they are, floats in the handle dtype; J0 / J_trial in double when supplied) and guarded outputs"""
    B, nu, tdt = gm.batch, gm.spec.nu, tdt_of(gm); n, P = 2 * nu, gm.batch // T
    ins = {k: dev(inp[k], None if inp[k].dtype == np.int32 else tdt) for k in ("X", "U", "status", "alpha", "dV", "ok", "Xcur", "Ucur") if k not in omit}
    shapes = {"J_trial": ((T, P), torch.float64), "J_cur": ((P,), torch.float64), "J_acc": ((P,), torch.float64), "choice": ((P,), torch.int32),
              "alpha_acc": ((P,), tdt), "X_new": ((H + 1, P, n), tdt), "U_new": ((H, P, nu), tdt)}
    outs = {k: guarded(s, t) for k, (s, t) in shapes.items() if k not in omit}
    if supplied is not None:
        ins["J0"] = dev(supplied[1]); outs["J_trial"] = dev(supplied[0])        # (an input in this mode: a plain tensor)
    cost = None if supplied is not None else {k: dev(inp[k], tdt) for k in ("Q", "R", "Qf", "goal")}
    return ins, outs, cost


def launch_select(gm, H, T, ins, outs, cost, act_off, m, c1=LC.C1, per_problem=0):
    ls = api.DojoLineSearch(*[api.addr(ins.get(k)) for k in LS_IN], *[api.addr(outs.get(k)) for k in LS_OUT], float(c1), int(act_off), int(m))
    qc = None if cost is None else api.DojoQuadraticCost(*[api.addr(cost.get(k)) for k in ("Q", "R", "Qf", "goal")], per_problem)
    return api.lib().dojo_linesearch_select_dev(gm.h, int(H), int(T), None if qc is None else C.byref(qc), C.byref(ls), api.torch_stream())


def run_select(gm, shape, H, T, inp, supplied=None, omit=()):
    _, n, nu, act_off, m = MC.SHAPES[shape]
    ins, outs, cost = select_buffers(gm, H, T, inp, supplied, omit)
    api._chk(launch_select(gm, H, T, ins, outs, cost, act_off, m))
    torch.cuda.synchronize()
    res = {}
    for k, t in outs.items():
        if supplied is None or k != "J_trial":
            assert guards_intact(t), k
        res[k] = t.cpu().numpy()
    return res


def check_select(res, ref, e, what):
    assert_same((what, "choice"), res["choice"], ref["choice"])
    assert_same((what, "alpha_acc"), res["alpha_acc"], ref["alpha"].astype(res["alpha_acc"].dtype))
    tio = res["alpha_acc"].dtype
    if "X_new" in res:
        assert_same((what, "X_new"), res["X_new"], ref["X"].astype(tio))
    if "U_new" in res:
        assert_same((what, "U_new"), res["U_new"], ref["U"].astype(tio))
    for k in LC.COSTS:
        if k not in res:
            continue
        got, want = res[k], ref[k]
        assert got.dtype == np.float64 and got.shape == want.shape
        assert (np.isnan(got) == np.isnan(want)).all(), (what, k)
        err, lim = float(np.nanmax(np.abs(got - want))), LC.bound(want, e[k])
        print("%s %s: max err %.3e, bound %.3e" % (what, k, err, lim))
        assert err <= lim, (what, k, err, lim)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,H,T,P", LC.CASES, ids=IDS)
def test_select_against_the_reference(shape, H, T, P, dtype):
    inp, _, ref, e = LC.reference(shape, H, T, P, dtype == "f32")
    gm = handle(shape, dtype, T * P)
    res = run_select(gm, shape, H, T, inp)
    check_select(res, ref, e, (shape, H, T, P, dtype))
    again = run_select(gm, shape, H, T, inp)                    # bit-identical from run to run
    for k in res:
        assert_same(("second run", k), again[k], res[k])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,H,T,P", [("cartpole1", 3, 8, 65), ("ant", 3, 9, 5), ("atlas", 2, 3, 5)])
def test_supplied_costs_give_the_choice_of_the_cost_mode(shape, H, T, P, dtype):
    inp, _, ref, e = LC.reference(shape, H, T, P, dtype == "f32")
    gm = handle(shape, dtype, T * P)
    own = run_select(gm, shape, H, T, inp)
    fed = run_select(gm, shape, H, T, inp, supplied=(own["J_trial"], own["J_cur"]))
    for k in ("choice", "alpha_acc", "X_new", "U_new", "J_acc", "J_cur"):
        assert_same(("supplied", k), fed[k], own[k])
    assert_same("J_trial is left alone", fed["J_trial"], own["J_trial"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,H,T", [("cartpole2", 3, 3), ("ant", 3, 9), ("slider", 1, 8)])
def test_select_does_not_depend_on_the_number_of_problems(shape, H, T, dtype):
    """P = 5 against the first 5 problems of P = 65: the same bits (the inputs are seeded per problem)"""
    f32 = dtype == "f32"
    small = run_select(handle(shape, dtype, T * 5), shape, H, T, LC.inputs(shape, H, T, 5, f32)[0])
    large = run_select(handle(shape, dtype, T * 65), shape, H, T, LC.inputs(shape, H, T, 65, f32)[0])
    for k in small:
        first = large[k][:, :5] if k in ("J_trial", "X_new", "U_new") else large[k][:5]
        assert_same((k, "P = 5 in P = 65"), small[k], first)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_select_optional_members(dtype):
    shape, H, T, P = "ant", 3, 9, 5
    _, n, nu, act_off, m = MC.SHAPES[shape]
    inp, _, ref, e = LC.reference(shape, H, T, P, dtype == "f32")
    gm = handle(shape, dtype, T * P)
    full = run_select(gm, shape, H, T, inp)
    for gone in ("J_cur", "X_new", "U_new"):                  # an output that is not wanted: the others are what they were
        res = run_select(gm, shape, H, T, inp, omit=(gone,))
        assert gone not in res
        for k in res:
            assert_same((gone, k), res[k], full[k])
    # status NULL: all solved; ok NULL: every problem may accept -- the reference without them
    for gone, kw in (("status", {"use_status": False}), ("ok", {"use_ok": False})):
        want = LC.select(inp, shape, T, np.longdouble, **kw)
        res = run_select(gm, shape, H, T, inp, omit=(gone,))
        check_select(res, {k: (np.asarray(v, dtype=np.float64) if k in LC.COSTS + ("alpha",) else v) for k, v in want.items()}, e, "no " + gone)
    # J0 given with a cost: it is used as it is (twice the computed one: every trial of a problem that may accept is acceptable)
    ins, outs, cost = select_buffers(gm, H, T, inp)
    ins["J0"] = dev(2.0 * full["J_cur"])
    api._chk(launch_select(gm, H, T, ins, outs, cost, act_off, m))
    torch.cuda.synchronize()
    assert_same("J_cur = J0 as given", outs["J_cur"].cpu().numpy(), 2.0 * full["J_cur"])
    assert_same("J_trial", outs["J_trial"].cpu().numpy(), full["J_trial"])
    want = LC.select(inp, shape, T, np.float64, J_trial=full["J_trial"], J0=2.0 * full["J_cur"])
    assert_same("choice under the given J0", outs["choice"].cpu().numpy(), want["choice"])
    # goal per problem: the shared goal repeated gives the same bits
    ins, outs, cost = select_buffers(gm, H, T, inp)
    cost["goal"] = cost["goal"][None].repeat(P, 1).contiguous()
    api._chk(launch_select(gm, H, T, ins, outs, cost, act_off, m, per_problem=1))
    torch.cuda.synchronize()
    for k in full:
        assert_same(("goal per problem", k), outs[k].cpu().numpy(), full[k])


def test_select_refusals():
    shape, H, T, P = "cartpole1", 3, 3, 5
    _, n, nu, act_off, m = MC.SHAPES[shape]
    inp = LC.inputs(shape, H, T, P)[0]
    gm = handle(shape, "f64", T * P)
    ins, outs, cost = select_buffers(gm, H, T, inp)
    who = "dojo_linesearch_select_dev: "

    def refused(text, H_=H, T_=T, ins_=ins, outs_=outs, cost_=cost, **kw):
        assert launch_select(gm, H_, T_, ins_, outs_, cost_, kw.pop("act_off", act_off), kw.pop("m", m), **kw) == INVALID, text
        assert gm.last_error().startswith(who) and text in gm.last_error(), (text, gm.last_error())

    refused("H must be >= 1", H_=0)
    refused("T must be 1 .. 64", T_=0)
    refused("T must be 1 .. 64", T_=65)
    refused("B mod T != 0", T_=4)
    for k in ("X", "U", "alpha", "dV", "Xcur", "Ucur"):
        refused("X, U, alpha, dV, Xcur, Ucur, choice, alpha_acc and J_acc must not be NULL", ins_={j: v for j, v in ins.items() if j != k})
    for k in ("choice", "alpha_acc", "J_acc"):
        refused("X, U, alpha, dV, Xcur, Ucur, choice, alpha_acc and J_acc must not be NULL", outs_={j: v for j, v in outs.items() if j != k})
    refused("J_trial must not be NULL", outs_={j: v for j, v in outs.items() if j != "J_trial"})
    refused("J0 must not be NULL without a cost", cost_=None)
    for k in ("Q", "R", "Qf", "goal"):
        refused("Q, R, Qf and goal of the cost must not be NULL", cost_={j: v for j, v in cost.items() if j != k})
    refused("the cost must cover inputs", m=0)
    refused("the cost must cover inputs", act_off=-1)
    refused("the cost must cover inputs", act_off=2, m=1)
    refused("c1 must be finite", c1=float("nan"))
    refused("c1 must be finite", c1=float("inf"))
    ls = api.DojoLineSearch()
    assert api.lib().dojo_linesearch_select_dev(None, H, T, None, C.byref(ls), api.torch_stream()) == INVALID
    assert api.lib().dojo_linesearch_select_dev(gm.h, H, T, None, None, api.torch_stream()) == INVALID and who + "bad argument" in gm.last_error()
    torch.cuda.synchronize()
    for k, v in outs.items():                                 # nothing was launched
        assert guards_intact(v) and bool((v == -77).all() if v.dtype == torch.int32 else torch.isnan(v).all()), k


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_select_host_entry_equals_the_device_entry(dtype):
    shape, H, T, P = "ant", 3, 9, 5
    _, n, nu, act_off, m = MC.SHAPES[shape]
    inp = LC.inputs(shape, H, T, P, dtype == "f32")[0]
    gm = handle(shape, dtype, T * P)
    ref = run_select(gm, shape, H, T, inp)
    got = gm.linesearch_select(T, inp["X"], inp["U"], inp["alpha"], inp["dV"], inp["Xcur"], inp["Ucur"], cost=(inp["Q"], inp["R"], inp["Qf"], inp["goal"]),
                               status=inp["status"], ok=inp["ok"], c1=LC.C1, act_off=act_off, na=m)
    for a, b in (("choice", "choice"), ("alpha", "alpha_acc"), ("J_trial", "J_trial"), ("J_cur", "J_cur"), ("J_acc", "J_acc"), ("X", "X_new"), ("U", "U_new")):
        assert_same(("host entry", a), got[a], ref[b])
    fed = gm.linesearch_select(T, inp["X"], inp["U"], inp["alpha"], inp["dV"], inp["Xcur"], inp["Ucur"], status=inp["status"], ok=inp["ok"], J0=ref["J_cur"],
                               J_trial=ref["J_trial"], c1=LC.C1, act_off=act_off, na=m)
    for a, b in (("choice", "choice"), ("alpha", "alpha_acc"), ("J_acc", "J_acc"), ("X", "X_new"), ("U", "U_new")):
        assert_same(("host entry, supplied costs", a), fed[a], ref[b])
    with pytest.raises(api.DojoError, match="dojo_linesearch_select: c1 must be finite"):
        gm.linesearch_select(T, inp["X"], inp["U"], inp["alpha"], inp["dV"], inp["Xcur"], inp["Ucur"], J0=ref["J_cur"], J_trial=ref["J_trial"], c1=float("nan"),
                             act_off=act_off, na=m)


# ================================================================ the fan rollout ================================================================
def fan_case(shape, H, T, P, dtype):
    """per problem: the inputs of minimal_cases with Xbar (test_rollout_minimal_gpu.case), limits around Ubar[0], and alpha [T,P] = alpha_p 2^-tr"""
    _, n, nu, act_off, m = MC.SHAPES[shape]
    inp = dict(RM.case(shape, H, P, dtype))
    lo, hi = RB.rollout_limits(inp, act_off, m, dtype == "f32")
    alpha = (np.maximum(inp["alpha"], 0.25)[None] * 2.0 ** -np.arange(T)[:, None])
    inp["alpha"] = alpha.astype(np.float32).astype(np.float64) if dtype == "f32" else alpha
    return inp, lo, hi


def launch_fan(gm, H, T, dev_in, outs, act_off, m, lo, hi, A=None, Bm=None):
    t = api.DojoTracking(*[api.addr(dev_in.get(k)) for k in RM.INPUTS], *[api.addr(outs.get(k)) for k in ("X", "U_out", "status")], api.addr(A), api.addr(Bm), int(act_off), int(m))
    lim = api.DojoControlLimits(api.addr(lo), api.addr(hi))
    return api.lib().dojo_rollout_minimal_fan_dev(gm.h, int(H), int(T), C.byref(t), None if lo is None and hi is None else C.byref(lim), api.torch_stream())


def run_fan(gm, H, T, inp, act_off, m, lo, hi, omit=()):
    tdt = tdt_of(gm)
    dev_in = {k: dev(inp.get(k), tdt) for k in RM.INPUTS}
    outs = RM.outputs(gm, H, omit=omit)
    api._chk(launch_fan(gm, H, T, dev_in, outs, act_off, m, dev(lo, tdt), dev(hi, tdt)))
    torch.cuda.synchronize()
    res = {}
    for k, t in outs.items():
        assert guards_intact(t), k
        res[k] = t.cpu().numpy()
        assert not (res[k] == -77).any() if k == "status" else not np.isnan(res[k]).any(), k       # every element was written
    return res


def repeated(inp, T, lo, hi):
    """every reference member T times along the batch axis; alpha [T,P] is [B] already"""
    rep = lambda a, axis: None if a is None else np.ascontiguousarray(np.concatenate([a] * T, axis=axis))
    out = {k: rep(inp.get(k), 1) for k in ("Ubar", "Xbar", "K", "kff")}
    out["x0"] = rep(inp["x0"], 0); out["alpha"] = None if inp.get("alpha") is None else inp["alpha"].reshape(-1)
    return out, rep(lo, 0), rep(hi, 0)


def reference_rollout(gm, H, T, inp, act_off, m, lo, hi):
    big, blo, bhi = repeated(inp, T, lo, hi)
    if lo is None and hi is None:
        return RM.run(gm, big, act_off, m)
    tdt = tdt_of(gm)
    outs = RM.outputs(gm, H)
    api._chk(RB.launch_rollout(gm, H, {k: dev(big.get(k), tdt) for k in RM.INPUTS}, outs, act_off, m, dev(blo, tdt), dev(bhi, tdt)))
    torch.cuda.synchronize()
    assert all(guards_intact(t) for t in outs.values())
    return {k: t.cpu().numpy() for k, t in outs.items()}


FAN_CASES = [("cartpole1", 3, 3, 5, 0), ("cartpole1", 3, 8, 65, 1), ("cartpole1", 3, 8, 65, 3), ("ant", 3, 4, 5, 0), ("atlas", 2, 2, 5, 0)]


@pytest.mark.parametrize("limited", [True, False], ids=["limits", "nolimits"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,H,T,P,groups", FAN_CASES, ids=["%s-H%d-T%d-P%d-g%d" % c for c in FAN_CASES])
def test_fan_is_the_rollout_of_the_repeated_inputs(shape, H, T, P, groups, dtype, limited):
    """X, U_out, status bit for bit; with dojo_set_groups(3) on T P = 520 environments the groups begin and end inside trials"""
    _, n, nu, act_off, m = MC.SHAPES[shape]
    inp, lo, hi = fan_case(shape, H, T, P, dtype)
    if not limited:
        lo = hi = None
    gm = handle(shape, dtype, T * P)
    gm.set_groups(groups)
    try:
        got = run_fan(gm, H, T, inp, act_off, m, lo, hi)
        gm.set_groups(0)
        ref = reference_rollout(gm, H, T, inp, act_off, m, lo, hi)
    finally:
        gm.set_groups(0)
    RM.same_outputs(got, ref, (shape, H, T, P, groups, dtype, limited))
    X0 = got["X"][0].reshape(T, P, n)
    assert all((X0[tr] == inp["x0"].astype(X0.dtype)).all() for tr in range(T))          # the broadcast of x0
    if T > 1:
        assert (got["U_out"][:, :P] != got["U_out"][:, P:2 * P]).any()                  # the trials differ: alpha does something
    if limited:
        u = got["U_out"][:, :, act_off:act_off + m].reshape(H, T, P, m).astype(np.float64)
        assert (u >= lo[None, None]).all() and (u <= hi[None, None]).all() and ((u == lo[None, None]) | (u == hi[None, None])).any()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fan_optional_members(dtype):
    shape, H, T, P = "cartpole2", 3, 3, 5
    _, n, nu, act_off, m = MC.SHAPES[shape]
    inp, lo, hi = fan_case(shape, H, T, P, dtype)
    gm = handle(shape, dtype, T * P)
    for gone in ("Ubar", "Xbar", "K", "kff", "alpha"):
        part = dict(inp, **{gone: None})
        RM.same_outputs(run_fan(gm, H, T, part, act_off, m, lo, hi), reference_rollout(gm, H, T, part, act_off, m, lo, hi), "no " + gone)
    RM.same_outputs(run_fan(gm, H, T, inp, act_off, m, lo, None), reference_rollout(gm, H, T, inp, act_off, m, lo, None), "lo alone")
    RM.same_outputs(run_fan(gm, H, T, inp, act_off, m, None, hi), reference_rollout(gm, H, T, inp, act_off, m, None, hi), "hi alone")
    full = run_fan(gm, H, T, inp, act_off, m, lo, hi)
    part = run_fan(gm, H, T, inp, act_off, m, lo, hi, omit=("status",))
    assert "status" not in part
    RM.same_outputs(part, {k: v for k, v in full.items() if k != "status"}, "no status")


def test_fan_refusals():
    shape, H, T, P = "cartpole1", 3, 3, 5
    _, n, nu, act_off, m = MC.SHAPES[shape]
    inp, lo, hi = fan_case(shape, H, T, P, "f64")
    gm = handle(shape, "f64", T * P)
    tdt = tdt_of(gm)
    dev_in = {k: dev(inp.get(k), tdt) for k in RM.INPUTS}
    outs = RM.outputs(gm, H)
    dlo, dhi = dev(lo, tdt), dev(hi, tdt)
    who = "dojo_rollout_minimal_fan_dev: "
    A = guarded((H, T * P, n, n), tdt); Bm = guarded((H, T * P, n, nu), tdt)
    for text, kw in (("T must be >= 1", dict(T=0)), ("B mod T != 0", dict(T=4)), ("H must be >= 1", dict(H=0)),
                     ("A and Bm must be NULL", dict(A=A, Bm=Bm)), ("A and Bm must both be given or both be NULL", dict(A=A)),
                     ("x0, X and U_out must not be NULL", dict(dev_in=dict(dev_in, x0=None))), ("the controller must drive inputs", dict(m=0))):
        args = dict(H=H, T=T, dev_in=dev_in, m=m, A=None, Bm=None); args.update(kw)
        assert launch_fan(gm, args["H"], args["T"], args["dev_in"], outs, act_off, args["m"], dlo, dhi, args["A"], args["Bm"]) == INVALID, text
        assert gm.last_error().startswith(who) and text in gm.last_error(), (text, gm.last_error())
    torch.cuda.synchronize()
    for k, v in list(outs.items()) + [("A", A), ("Bm", Bm)]:
        assert guards_intact(v) and bool((v == -77).all() if k == "status" else torch.isnan(v).all()), k
    bad = hi.copy(); bad[2, 0] = lo[2, 0] - 1.0
    with pytest.raises(api.DojoError, match="dojo_rollout_minimal_fan: the limits must satisfy lo <= hi"):
        gm.rollout_minimal_fan(T, inp["x0"], lo=lo, hi=bad, Ubar=inp["Ubar"], Xbar=inp["Xbar"], K=inp["K"], kff=inp["kff"], alpha=inp["alpha"], act_off=act_off, na=m)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fan_host_entry_equals_the_device_entry(dtype):
    shape, H, T, P = "ant", 3, 4, 5
    _, n, nu, act_off, m = MC.SHAPES[shape]
    inp, lo, hi = fan_case(shape, H, T, P, dtype)
    gm = handle(shape, dtype, T * P)
    for l, h in ((lo, hi), (None, None)):
        ref = run_fan(gm, H, T, inp, act_off, m, l, h)
        X, U, st = gm.rollout_minimal_fan(T, inp["x0"], lo=l, hi=h, Ubar=inp["Ubar"], Xbar=inp["Xbar"], K=inp["K"], kff=inp["kff"], alpha=inp["alpha"], act_off=act_off, na=m)
        RM.same_outputs(ref, {"X": X, "U_out": U, "status": st}, "host entry")


# ================================================================ the driver ================================================================
DT = torch.float64
ALPHAS = (1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125)          # those of ilqr.solve


def cartpole_pair(P, dtype, T=len(ALPHAS)):
    opts = d.SolverOptions(rtol=1e-8, btol=1e-8) if dtype == "f64" else None
    return (api.BatchedMechanism(d.get_cartpole(), P, dtype=dtype, opts=opts), api.BatchedMechanism(d.get_cartpole(), T * P, dtype=dtype, opts=opts))


def test_side_by_side_is_solve_limited_on_the_cartpole():
    """f64, P = 5, the swing-up start and the cost of the iLQR tests, 3 iterations under |u| <= F: the same step lengths, U and X bit for bit -- provided no
    trial's cost lies within 1e-9 max(1, |J|) of its threshold, which is asserted first.  The loop runs without a device-to-host read."""
    P, H, iters = 5, 30, 3
    gm, gmt = cartpole_pair(P, "f64")
    try:
        x0, cost = RB.cartpole_problem(P)
        U0 = torch.zeros((H, P, 2), dtype=DT, device="cuda")
        # the limit of test_solve_limited_on_the_cartpole: half of the largest |u| the unconstrained solve reaches.  (Under |u| <= 5 this test's margin
        # condition was missed on an MI355X: smallest distance 0.000e+00 in the third iteration, choices [[0, 0, 0, 0, 1], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]] -- a
        # problem whose every step is clamped has kff = K = 0 and dV = 0, so every trial is the current trajectory and its cost EQUALS its threshold.)
        F = 0.5 * float(ilqr.solve(gm, x0, U0, cost, 6, act_off=0, na=1)["U"][:, :, 0].abs().max())
        ref = ilqr.solve_limited(gm, x0, U0, cost, iters, -F, F, act_off=0, na=1, fused=True)
        lo, hi = torch.full((P, 1), -F, dtype=DT, device="cuda"), torch.full((P, 1), F, dtype=DT, device="cuda")      # (made outside the loop under test)
        alphas = torch.tensor(ALPHAS, dtype=DT, device="cuda")
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")          # a synchronizing call inside the loop raises (the mode works on torch for ROCm: an upload from pageable memory trips it)
        try:
            res = ilqr.solve_side_by_side(gm, gmt, x0, U0, cost, iters, lo, hi, act_off=0, na=1, alphas=alphas)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        J, Jt, dV = res["J"][:-1].cpu().numpy(), res["J_trial"].cpu().numpy(), res["dV"].cpu().numpy()
        a = np.array(ALPHAS)[None, :, None]
        thr = J[:, None] + 1e-4 * (a * dV[:, None, :, 0] + a * a * dV[:, None, :, 1])
        dist = np.abs(Jt - thr) / np.maximum(1.0, np.abs(J))[:, None]
        print("smallest distance of a trial from its threshold: %.3e; choices %s" % (float(np.nanmin(dist)), res["choice"].cpu().numpy().tolist()))
        assert float(np.nanmin(dist)) >= 1e-9
        assert torch.equal(res["a"], ref["a"]) and bool((res["a"] > 0).any())
        assert torch.equal(res["U"], ref["U"]) and torch.equal(res["X"], ref["X"])
        assert torch.equal(res["active"], ref["active"]) and torch.equal(res["mu"], ref["mu"]) and torch.equal(res["fail"], ref["fail"])
        assert res["choice"].shape == (iters, P) and res["J_trial"].shape == (iters, len(ALPHAS), P) and res["J_trial"].dtype == torch.float64
        assert np.abs(res["J"].cpu().numpy() - ref["J"].cpu().numpy()).max() <= 1e-12 * np.abs(ref["J"].cpu().numpy()).max()
        assert set(res) == set(ref) | {"choice", "J_trial"}
    finally:
        gm.close(); gmt.close()


def test_side_by_side_costs_never_rise_on_the_f32_cartpole():
    P, H, iters = 5, 30, 4
    gm, gmt = cartpole_pair(P, "f32")
    try:
        x0, cost = RB.cartpole_problem(P)
        f = lambda t: t.to(torch.float32)
        cost = ilqr.QuadraticCost(f(cost.Q), f(cost.R), f(cost.Qf), f(cost.g))
        res = ilqr.solve_side_by_side(gm, gmt, f(x0), torch.zeros((H, P, 2), dtype=torch.float32, device="cuda"), cost, iters, act_off=0, na=1)
        torch.cuda.synchronize()
        J, a = res["J"].cpu().numpy(), res["a"].cpu().numpy()
        assert J.dtype == np.float64 and np.isfinite(J).all() and (a > 0).any()
        assert (np.diff(J[:-1], axis=0) <= 0).all(), J          # the costs of the accepted trajectories, as the kernel evaluated them
        assert (np.diff(J[:-1], axis=0)[a[:-1] == 0] == 0).all()
        assert (J[-1] <= J[0]).all()

        class Opaque:                      # any other cost object: evaluated by cost.value and handed over as J_trial
            value, quadratize = cost.value, cost.quadratize
        other = ilqr.solve_side_by_side(gm, gmt, f(x0), torch.zeros((H, P, 2), dtype=torch.float32, device="cuda"), Opaque(), 2, act_off=0, na=1)
        torch.cuda.synchronize()
        assert np.isfinite(other["J"].cpu().numpy()).all() and bool((other["choice"] >= -1).all())
    finally:
        gm.close(); gmt.close()


def test_side_by_side_solves_the_slider_in_one_iteration():
    """linear dynamics, quadratic cost: the full step is the optimum -- choice = 0, and a second iteration changes nothing to speak of"""
    P, H, T = 5, 10, 3
    spec = d.get_mechanism("slider")
    gm, gmt = api.BatchedMechanism(spec, P, dtype="f64", opts=d.SolverOptions(rtol=1e-10, btol=1e-10)), api.BatchedMechanism(spec, T * P, dtype="f64", opts=d.SolverOptions(rtol=1e-10, btol=1e-10))
    try:
        x0 = torch.zeros((P, 2), dtype=DT, device="cuda"); x0[:, 0] = torch.linspace(0.1, 0.5, P, dtype=DT, device="cuda")
        cost = ilqr.QuadraticCost(torch.eye(2, dtype=DT, device="cuda"), 0.1 * torch.eye(1, dtype=DT, device="cuda"), 10.0 * torch.eye(2, dtype=DT, device="cuda"),
                                  torch.tensor([1.0, 0.0], dtype=DT, device="cuda"))
        res = ilqr.solve_side_by_side(gm, gmt, x0, torch.zeros((H, P, 1), dtype=DT, device="cuda"), cost, 2, alphas=(1.0, 0.5, 0.25))
        torch.cuda.synchronize()
        J = res["J"].cpu().numpy()
        assert (res["choice"][0] == 0).all() and (res["a"][0] == 1.0).all()
        assert (J[1] < J[0]).all() and (np.abs(J[2] - J[1]) <= 1e-6 * np.abs(J[1])).all()
    finally:
        gm.close(); gmt.close()


def test_example_runs_side_by_side():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "dojo.jl_amd", "host")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cartpole_ilqr_device.py"), "8", "20", "4", "--side-by-side"],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "side by side" in out.stdout
