"""The reference of the control-limited backward pass (tests/box_cases.py) pinned without a device: against an independent brute-force solution of the step's
QP, against riccati_cases.recursion at infinite limits, and the conditions on the inputs that the GPU test relies on -- the clamped set is only determined where
the solution is strictly complementary, so every case the GPU test uses must have a margin, the same set in fp64 and in longdouble, and no failure."""
import numpy as np
import pytest

import box_cases as BC
import minimal_cases as MC
import riccati_cases as RC

SMALL = [c for c in BC.CASES if RC.SHAPES[c[0]][4] <= 8]


@pytest.mark.parametrize("c", BC.CS)
@pytest.mark.parametrize("shape,H,B", SMALL)
def test_brute_force_agrees_on_the_last_two_steps(shape, H, B, c):
    """m <= 8: kff and the clamped set of the reference equal the enumeration of all 3^m active patterns, to 1e-9 relative, at the last two steps of two environments"""
    _, n, nu, act_off, m = RC.SHAPES[shape]
    inp, U, lo, hi, ref, e, r64 = BC.reference(shape, H, B, c)
    for b in (0, B - 1):
        for k in (H - 1, H - 2):
            Qreg, Qu = BC.step_model(inp, ref, act_off, m, k, b)
            u = U[k, b, act_off:act_off + m]
            x, cl = BC.brute_force(Qreg, Qu, lo[b] - u, hi[b] - u)
            assert np.array_equal(cl, ref["mask"][k, b]), (shape, k, b)
            assert np.abs(x - ref["kff"][k, b]).max() <= 1e-9 * max(1.0, np.abs(x).max()), (shape, k, b)
            assert ref["active"][k, b] == sum(1 << i for i in range(m) if cl[i])


@pytest.mark.parametrize("shape,H,B", [("cartpole2", 3, 5), ("ant", 3, 5), ("atlas5", 3, 5)])
def test_infinite_limits_reproduce_the_unconstrained_recursion_exactly(shape, H, B):
    _, n, nu, act_off, m = RC.SHAPES[shape]
    inp = RC.inputs(shape, H, B)
    U = BC.controls(shape, H, B, BC.C_MAIN)
    plain = RC.recursion(inp, act_off, m)
    inf = np.full((B, m), np.inf)
    for lo, hi in ((-inf, inf), (None, None), (-inf, None)):
        out = BC.recursion(inp, U, lo, hi, act_off, m)
        for k in ("K", "kff", "dV", "Vx", "Vxx", "fail"):
            assert np.array_equal(out[k], plain[k]), k
        assert not out["iters"].any() and not out["active"].any() and not out["mask"].any()


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("c", BC.CS)
@pytest.mark.parametrize("shape,H,B", BC.GPU_CASES)
def test_conditions_on_the_inputs_of_the_gpu_test(shape, H, B, c, f32):
    """conditions, not measurements: the fp64 and the longdouble run clamp the same sets and do not fail, the margin is >= 1e-6, and at c = 0.25 at least a quarter
    of all inputs are clamped with no QP over 8 iterations"""
    inp, U, lo, hi, ref, e, r64 = BC.reference(shape, H, B, c, f32)
    assert not ref["fail"].any() and not r64["fail"].any()
    assert np.array_equal(ref["mask"], r64["mask"]) and np.array_equal(ref["active"], r64["active"])
    assert min(ref["margin"].min(), r64["margin"].min()) >= 1e-6
    assert (np.abs(U) <= c).all() and (np.abs(U) == c).any()
    print("%s H=%d B=%d c=%g f32=%s: clamped share %.2f, iterations <= %d, margin %.1e, e_ref %.1e"
          % (shape, H, B, c, f32, ref["mask"].mean(), max(ref["iters"].max(), r64["iters"].max()), ref["margin"].min(), max(e.values())))
    if c == BC.C_MAIN:
        assert ref["mask"].mean() >= 0.25
        assert max(ref["iters"].max(), r64["iters"].max()) <= 8
    # clamped rows: zero gain, kff on the bound; nothing clamped: no iteration
    assert not ref["K"][ref["mask"]].any()
    m, act_off = RC.SHAPES[shape][4], RC.SHAPES[shape][3]
    x = ref["kff"] + U[:, :, act_off:act_off + m]
    assert (np.abs(np.abs(x[ref["mask"]]) - c) <= 1e-15).all() and (np.abs(x) <= c * (1 + 1e-15)).all()
    assert not ref["iters"][~ref["mask"].any(-1)].any()


def test_failure_codes_of_the_reference():
    _, n, nu, act_off, m = RC.SHAPES["ant"]
    H, B = 4, 3
    inp = RC.inputs("ant", H, B); U = BC.controls("ant", H, B, BC.C_MAIN); lo, hi = BC.limits("ant", B, BC.C_MAIN)
    bad = lo.copy(); bad[1, 3] = 1.0                              # lo > hi
    out = BC.recursion(inp, U, bad, hi, act_off, m)
    assert out["fail"].tolist() == [0, -H, 0] and not out["K"][:, 1].any() and not out["Vxx"][1].any()
    bad = hi.copy(); bad[1, 0] = np.nan
    assert BC.recursion(inp, U, lo, bad, act_off, m)["fail"].tolist() == [0, -H, 0]
    p = {k: v.copy() for k, v in inp.items()}; p["luu"][2, 1] = -1.0e4 * np.eye(m)
    out = BC.recursion(p, U, lo, hi, act_off, m)
    assert out["fail"].tolist() == [0, 3, 0] and not out["active"][:3, 1].any() and out["K"][3, 1].any()


@pytest.mark.parametrize("shape", ["slider", "cartpole2", "ant"])
def test_clamping_before_the_rounding_equals_clamping_after_it(shape):
    """the clamped law: minimal_cases.law, then np.clip into limits that are fp32 values -- the same fp32 result whether the clip comes before or after the rounding"""
    name, n, nu, act_off, m = MC.SHAPES[shape]
    H, B = 3, 65
    inp = dict(MC.inputs(shape, H, B, f32=True), Xbar=None)
    rng = np.random.default_rng(5)
    X = (inp["x0"] + 0.3 * rng.standard_normal(inp["x0"].shape)).astype(np.float32).astype(np.float64)
    hits = 0
    for k in range(H):
        u, _ = MC.law(inp, k, X, act_off, m, np.float64)
        a = u[:, act_off:act_off + m]
        for c in (np.float32(0.05), np.float32(0.1), np.float32(0.3)):
            lo, hi = -float(c), float(c)
            before = np.clip(a, lo, hi).astype(np.float32)
            after = np.clip(a.astype(np.float32), np.float32(lo), np.float32(hi))
            assert before.tobytes() == after.tobytes()
            hits += int((np.abs(before) == c).sum())
    assert hits > 0
