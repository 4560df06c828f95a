"""The NumPy reference of the constrained backward pass (tests/al_cases.py) against independent statements of the same mathematics, and the conditions the GPU
gate of tests/test_riccati_al_gpu.py relies on.  No device."""
import numpy as np
import pytest

import al_cases as AC
import box_cases as BC
import riccati_cases as RC

SMALL = [("slider", 3, 5), ("cartpole1", 3, 5), ("cartpole2", 3, 5), ("ant", 3, 5)]


@pytest.mark.parametrize("shape,H,B", SMALL)
def test_folding_the_terms_into_the_cost_gives_the_same_outputs(shape, H, B):
    """lxx + Cx' w Cx etc. formed in memory and handed to the box recursion: the same outputs within the fp64-against-longdouble error of the case"""
    _, n, nu, act_off, m = RC.SHAPES[shape]
    inp, con, U, lo, hi, ref, e, r64 = AC.reference(shape, H, B)
    got = BC.recursion(AC.folded(inp, con, m), np.zeros((H, B, nu)), None, None, act_off, m)
    assert not got["fail"].any()
    for k in AC.OUTPUTS:
        assert np.abs(got[k] - ref[k]).max() <= RC.bound(ref[k], e[k], False), k


@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("shape,H,B", SMALL)
def test_dead_rows_change_nothing_at_all(shape, H, B, limited):
    """w = y = 0 everywhere (NaN in every Jacobian), and nc = 0: the difference from the box recursion is exactly 0"""
    _, n, nu, act_off, m = RC.SHAPES[shape]
    inp = RC.inputs(shape, H, B)
    U = BC.controls(shape, H, B, BC.C_MAIN); lo, hi = BC.limits(shape, B, BC.C_MAIN) if limited else (None, None)
    box = BC.recursion(inp, U, lo, hi, act_off, m)
    con = AC.constraints(shape, H, B)
    dead = {"Cx": np.full_like(con["Cx"], np.nan), "Cu": np.full_like(con["Cu"], np.nan), "w": np.zeros_like(con["w"]), "y": np.zeros_like(con["y"])}
    for c in (dead, AC.constraints(shape, H, B, nc=0), None):
        got = AC.recursion(inp, c, act_off, m, U, lo, hi)
        for k in box:
            assert np.array_equal(got[k], box[k]), k
    assert limited == bool(box["active"].any())


def lq_problem(seed, H=6, n=4, m=2, nc=3):
    rng = np.random.default_rng(seed)
    A = np.eye(n) + 0.2 * rng.standard_normal((H, n, n)); Bm = rng.standard_normal((H, n, m)); aff = 0.1 * rng.standard_normal((H, n))
    M = rng.standard_normal((n, n)); Q = M @ M.T + 0.1 * np.eye(n)
    M = rng.standard_normal((m, m)); R = M @ M.T + np.eye(m)
    M = rng.standard_normal((n, n)); Qf = M @ M.T + 0.1 * np.eye(n)
    x0, xg = rng.standard_normal(n), rng.standard_normal(n)
    Cx = rng.standard_normal((nc, n)); d = rng.standard_normal(nc)
    return A, Bm, aff, Q, R, Qf, x0, xg, Cx, d


def rollout(A, Bm, aff, x0, U):
    X = [x0]
    for k in range(len(U)):
        X.append(A[k] @ X[k] + Bm[k] @ U[k] + aff[k])
    return np.stack(X)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_predicted_change_of_the_merit_equals_the_actual_one(seed):
    """an LQ problem, equality rows at every stage, multipliers and weights frozen: M(a) - M(0) = a dV[0] + a^2 dV[1] for the closed-loop step of length a, where
    M = J + sum lam c + 1/2 sum w c^2 and y = lam + w c"""
    A, Bm, aff, Q, R, Qf, x0, xg, Cx, d = lq_problem(seed)
    H, n, m = Bm.shape; nc = len(d)
    rng = np.random.default_rng([seed, 7])
    U = rng.standard_normal((H, m)); X = rollout(A, Bm, aff, x0, U)
    lam = rng.standard_normal((H + 1, nc)); w = 10.0 ** rng.uniform(-1, 2, (H + 1, nc)); w[2] = 0.0; lam[2] = 0.0      # a stage of dead rows
    Cu = rng.standard_normal((H, nc, m))

    def merit(X, U):
        c = X @ Cx.T - d; c[:-1] += np.einsum("kij,kj->ki", Cu, U)
        return AC.lq_cost(X, U, Q, R, Qf, xg) + (lam * c).sum() + 0.5 * (w * c * c).sum(), c

    M0, c = merit(X, U)
    dx = X - xg
    inp = {"A": A[:, None], "Bm": Bm[:, None], "lx": np.concatenate([dx[:-1] @ Q.T, (dx[-1] @ Qf.T)[None]])[:, None], "lu": (U @ R.T)[:, None],
           "lxx": np.concatenate([np.broadcast_to(Q, (H, n, n)), Qf[None]])[:, None], "luu": np.broadcast_to(R, (H, 1, m, m)), "lux": None}
    con = {"Cx": np.broadcast_to(Cx, (H + 1, 1, nc, n)), "Cu": Cu[:, None], "w": w[:, None], "y": (lam + w * c)[:, None]}
    r = AC.recursion(inp, con, 0, m)
    assert r["fail"][0] == 0
    for a in (1.0, 0.5, 0.125):
        Xa, Ua = X.copy(), U.copy()
        for k in range(H):
            Ua[k] = U[k] + a * r["kff"][k, 0] + r["K"][k, 0] @ (Xa[k] - X[k])
            Xa[k + 1] = A[k] @ Xa[k] + Bm[k] @ Ua[k] + aff[k]
        Ma, _ = merit(Xa, Ua)
        pred = a * r["dV"][0, 0] + a * a * r["dV"][0, 1]
        assert pred < 0 and abs((Ma - M0) - pred) <= 1e-10 * max(1.0, abs(M0)), (a, Ma - M0, pred)


@pytest.mark.parametrize("seed", [0, 1])
def test_the_al_loop_converges_to_the_kkt_solution(seed):
    """an LQ problem with a terminal equality: the limit of the augmented-Lagrangian loop is the dense KKT solution"""
    A, Bm, aff, Q, R, Qf, x0, xg, Cx, d = lq_problem(seed)
    H, n, m = Bm.shape; nc = len(d)
    U0 = np.zeros((H, m)); X0 = rollout(A, Bm, aff, x0, U0)
    present = np.zeros((H + 1, nc), bool); present[H] = True
    res = AC.al_loop_lq(A, Bm, X0, U0, Q, R, Qf, xg, Cx, d, np.zeros(nc, bool), present, outer=8)
    Xk, Uk = AC.kkt_lq(A, Bm, x0, aff, Q, R, Qf, xg, Cx, d)
    assert np.abs(Cx @ Xk[-1] - d).max() <= 1e-10
    assert res["viol"][-1] <= 1e-9 and res["viol"][-1] < res["viol"][1] < res["viol"][0]
    assert np.abs(res["U"] - Uk).max() <= 1e-7 * max(1.0, np.abs(Uk).max()) and np.abs(res["X"] - Xk).max() <= 1e-7 * max(1.0, np.abs(Xk).max())
    assert np.abs(res["X"] - rollout(A, Bm, aff, x0, res["U"])).max() <= 1e-9 * max(1.0, np.abs(Xk).max())      # the loop's delta updates follow the dynamics


def test_inequality_rows_of_the_al_loop_end_feasible_with_nonnegative_multipliers():
    """x_H[0] <= d with the goal beyond d: the bound ends active, lam > 0; with the goal inside it never activates, lam = 0 and the unconstrained optimum stands"""
    A, Bm, aff, Q, R, Qf, x0, xg, _, _ = lq_problem(3)
    H, n, m = Bm.shape
    Cx = np.zeros((1, n)); Cx[0, 0] = 1.0
    U0 = np.zeros((H, m)); X0 = rollout(A, Bm, aff, x0, U0)
    present = np.zeros((H + 1, 1), bool); present[H] = True
    free = AC.al_loop_lq(A, Bm, X0, U0, Q, R, Qf, xg, Cx, np.array([1e6]), np.ones(1, bool), present, outer=3)
    assert not free["lam"].any() and free["viol"].max() == 0.0
    d = np.array([free["X"][-1, 0] - 0.5])
    res = AC.al_loop_lq(A, Bm, X0, U0, Q, R, Qf, xg, Cx, d, np.ones(1, bool), present, outer=8)
    assert res["lam"][H, 0] > 0 and (res["lam"] >= 0).all() and res["viol"][-1] <= 1e-8 and abs(res["X"][-1, 0] - d[0]) <= 1e-8


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("shape,H,B", AC.CASES)
def test_conditions_of_the_gpu_gate(shape, H, B, f32):
    """per GPU case: no failure in either precision, e_ref <= 1e-13, w <= 1e3, and rows of every kind (dead, a multiplier without a weight, weighted)"""
    inp, con, U, lo, hi, ref, e, r64 = AC.reference(shape, H, B, f32)
    assert not ref["fail"].any() and not r64["fail"].any()
    assert max(e.values()) <= 1e-13, e
    assert con["w"].max() <= AC.W_MAX and con["w"].min() >= 0
    lv = AC.live(con["w"], con["y"])
    if con["w"].size >= 40:
        assert (~lv).any() and (lv & (con["w"] == 0)).any() and (con["w"] > 0).any()
    assert con["w"].shape[-1] == AC.NC[shape]


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("shape,H,B", AC.LIMITED_CASES)
def test_conditions_of_the_limited_gpu_cases(shape, H, B, f32):
    """limits and constraints together: the strict-complementarity margin of DESIGN.md 5j and identical clamped sets in both precisions"""
    inp, con, U, lo, hi, ref, e, r64 = AC.reference(shape, H, B, f32, limited=True)
    assert not ref["fail"].any() and not r64["fail"].any()
    assert max(e.values()) <= 1e-13, e
    assert np.array_equal(ref["mask"], r64["mask"]) and ref["mask"].any()
    assert min(ref["margin"].min(), r64["margin"].min()) >= 1e-6
