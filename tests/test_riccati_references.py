"""The NumPy reference of the Riccati backward pass (tests/riccati_cases.py), pinned on the CPU: it is well conditioned on every case the GPU test uses (fp64 against
longdouble), it solves the linear-quadratic problem it is meant to solve, its fixed point is the discrete algebraic Riccati equation's, and its failure
rules are the documented ones.  No device."""
import numpy as np
import pytest
import scipy.linalg

import riccati_cases as RC


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("shape,H,B", RC.CASES)
def test_reference_is_well_conditioned_on_the_gpu_cases(shape, H, B, f32):
    """e_ref = |fp64 - longdouble| / max|out| <= 1e-14 per output array: the gate of the GPU test (32 max(e_ref, 2^-52)) means nothing on an ill-conditioned case"""
    _, _, e = RC.reference(shape, H, B, f32)
    for k in RC.OUTPUTS:
        assert e[k] <= 1e-14, (k, e[k])


def lq_problem(n, nu, act_off, m, H, e=0):
    inp = RC.env_inputs(n, nu, act_off, m, H, e, seed=31)
    return {k: v[:, None] for k, v in inp.items()}           # a batch of one


def model_cost(p, act_off, m, X, U):
    """the quadratic model: sum_k lx.x + x'lxx x / 2 + lu.u + u'luu u / 2 + u'lux x, plus the terminal terms"""
    H = U.shape[0]
    J = p["lx"][H, 0] @ X[H] + 0.5 * X[H] @ p["lxx"][H, 0] @ X[H]
    for k in range(H):
        J += p["lx"][k, 0] @ X[k] + 0.5 * X[k] @ p["lxx"][k, 0] @ X[k] + p["lu"][k, 0] @ U[k] + 0.5 * U[k] @ p["luu"][k, 0] @ U[k] + U[k] @ p["lux"][k, 0] @ X[k]
    return J


def closed_loop(p, act_off, m, out, a=1.0):
    """x_{k+1} = A x + B u from x_0 = 0 under u = a kff + K x"""
    H, n = p["A"].shape[0], p["A"].shape[2]
    X = np.zeros((H + 1, n)); U = np.zeros((H, m))
    for k in range(H):
        U[k] = a * out["kff"][k, 0] + out["K"][k, 0] @ X[k]
        X[k + 1] = p["A"][k, 0] @ X[k] + p["Bm"][k, 0][:, act_off:act_off + m] @ U[k]
    return X, U


@pytest.mark.parametrize("n,nu,act_off,m,H", [(2, 1, 0, 1, 3), (4, 2, 0, 1, 40), (28, 14, 6, 8, 20), (36, 18, 6, 12, 20), (72, 36, 6, 30, 20), (6, 6, 0, 6, 5)])
def test_linear_quadratic_optimality(n, nu, act_off, m, H):
    """On a linear-quadratic problem one backward pass is the solution: the predicted change a dV[0] + a^2 dV[1] is the actual change of the cost for every
    step length a (the cost at x = 0, u = 0 is 0), and the gradient of the cost w.r.t. the controls vanishes at the closed-loop solution for a = 1."""
    p = lq_problem(n, nu, act_off, m, H)
    out = RC.recursion(p, act_off, m)
    assert out["fail"][0] == 0
    for a in (1.0, 0.5, 0.1):
        X, U = closed_loop(p, act_off, m, out, a)
        J = model_cost(p, act_off, m, X, U)
        pred = a * out["dV"][0, 0] + a * a * out["dV"][0, 1]
        assert abs(J - pred) <= 1e-11 * abs(out["dV"][0]).max(), (a, J, pred)
    # gradient w.r.t. U by the adjoint of the linear dynamics
    X, U = closed_loop(p, act_off, m, out, 1.0)
    lam = p["lx"][H, 0] + p["lxx"][H, 0] @ X[H]
    gmax, scale = 0.0, 0.0
    for k in range(H - 1, -1, -1):
        Bk = p["Bm"][k, 0][:, act_off:act_off + m]
        gu = p["lu"][k, 0] + p["luu"][k, 0] @ U[k] + p["lux"][k, 0] @ X[k] + Bk.T @ lam
        scale = max(scale, np.abs(p["lu"][k, 0]).max() + np.abs(p["luu"][k, 0] @ U[k]).max() + np.abs(Bk.T @ lam).max())
        gmax = max(gmax, np.abs(gu).max())
        lam = p["lx"][k, 0] + p["lxx"][k, 0] @ X[k] + p["lux"][k, 0].T @ U[k] + p["A"][k, 0].T @ lam
    assert gmax <= 1e-11 * scale, (gmax, scale)


def test_fixed_point_is_the_discrete_riccati_equation():
    """time-invariant A, B, Q, R over 400 steps: K_0 is scipy's DARE gain and Vxx its solution (A is a contraction, so that 400 steps are the fixed point whatever
    the pair (A, B) can reach: the closed loop decays at least as 0.8^k)"""
    n, m, H = 4, 1, 400
    rng = np.random.default_rng(5)
    A = 0.8 * (np.eye(n) + 0.1 * rng.standard_normal((n, n)) / np.sqrt(n)); Bm = rng.standard_normal((n, m)) / np.sqrt(n)
    M = rng.standard_normal((n, n)); Q = M @ M.T + 0.1 * np.eye(n); R = np.eye(m) * 1.5
    p = {"A": np.tile(A, (H, 1, 1, 1)), "Bm": np.tile(Bm, (H, 1, 1, 1)), "lx": np.zeros((H + 1, 1, n)), "lu": np.zeros((H, 1, m)),
         "lxx": np.tile(Q, (H + 1, 1, 1, 1)), "luu": np.tile(R, (H, 1, 1, 1)), "lux": None}
    out = RC.recursion(p, 0, m)
    P = scipy.linalg.solve_discrete_are(A, Bm, Q, R)
    K = -np.linalg.solve(R + Bm.T @ P @ Bm, Bm.T @ P @ A)
    assert out["fail"][0] == 0
    assert np.abs(out["K"][0, 0] - K).max() <= 1e-10 * np.abs(K).max()
    assert np.abs(out["Vxx"][0] - P).max() <= 1e-10 * np.abs(P).max()


def failure_inputs(shape="ant", H=5, B=3):
    """environment 1 of 3 carries the defect; a writable copy"""
    return {k: v.copy() for k, v in RC.inputs(shape, H, B).items()}


def env(out, k, b):
    """environment b of an output array (K, kff carry the step axis first)"""
    return out[k][:, b] if k in ("K", "kff") else out[k][b]


def test_failure_table():
    _, n, nu, act_off, m = RC.SHAPES["ant"]
    clean = RC.recursion(failure_inputs(), act_off, m)
    # luu_2 = -1e4 I: indefinite by a clear margin (B^T Vxx B is of the order of trace(Vxx) / n, some hundreds here) -> fail = 3; mu = 2e4 cures it
    p = failure_inputs(); p["luu"][2, 1] = -1.0e4 * np.eye(m)
    out = RC.recursion(p, act_off, m)
    assert out["fail"].tolist() == [0, 3, 0]
    assert not out["K"][:3, 1].any() and not out["kff"][:3, 1].any() and out["K"][3:, 1].all()
    assert not out["dV"][1].any() and not out["Vx"][1].any() and not out["Vxx"][1].any()
    for k in RC.OUTPUTS:
        np.testing.assert_array_equal(env(out, k, 0), env(clean, k, 0)); np.testing.assert_array_equal(env(out, k, 2), env(clean, k, 2))
    np.testing.assert_array_equal(out["K"][3:, 1], clean["K"][3:, 1])
    cured = RC.recursion(p, act_off, m, mu=np.array([0.0, 2.0e4, 0.0]))
    assert cured["fail"].tolist() == [0, 0, 0] and np.isfinite(cured["K"]).all()
    # a NaN in A of the solved step 3: Quu of step 3 does not see A_3, its K does; the value function is NaN from there and the pivot of step 2 fails
    p = failure_inputs(); p["A"][3, 1, 0, 0] = np.nan
    out = RC.recursion(p, act_off, m)
    assert out["fail"].tolist() == [0, 3, 0]
    assert not out["K"][:3, 1].any() and np.isnan(out["K"][3, 1]).any() and np.isfinite(out["K"][4, 1]).all()
    for b in (0, 2):
        for k in RC.OUTPUTS:
            np.testing.assert_array_equal(env(out, k, b), env(clean, k, b))


def test_failed_steps_are_not_read():
    """A_k, B_k of a step with status != 0 count as zero: NaN there changes nothing"""
    _, n, nu, act_off, m = RC.SHAPES["ant"]
    H, B = 5, 3
    status = np.zeros((H, B), np.int32); status[4, 0] = 1; status[0, 1] = 2; status[1:3, 2] = -1
    zeros = failure_inputs(H=H, B=B); nans = failure_inputs(H=H, B=B)
    for k in ("A", "Bm"):
        zeros[k][status != 0] = 0.0; nans[k][status != 0] = np.nan
    a, b = RC.recursion(zeros, act_off, m), RC.recursion(nans, act_off, m, status=status)
    assert not b["fail"].any()
    for k in RC.OUTPUTS:
        np.testing.assert_array_equal(a[k], b[k])
    free = RC.recursion(failure_inputs(H=H, B=B), act_off, m)
    assert np.abs(free["K"] - b["K"]).max() > 1e-3           # (and the failed steps do matter)
