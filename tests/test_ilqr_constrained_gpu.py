"""ilqr.solve_constrained on the GPU: IterativeLQR's augmented-Lagrangian loop around the device iLQR, the backward pass being dojo_riccati_al_dev
(include/dojo_hip_constraints.h).  The slider is affine, so its histories are compared with the NumPy loop of tests/al_cases.py; the cartpole is compared with the
unconstrained solve under the same cost."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import dojo_amd as d
from dojo_amd import api, ilqr

import al_cases as AC
import riccati_cases as RC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.float64
T = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=DT, device="cuda")


def test_slider_with_a_terminal_goal_follows_the_numpy_loop():
    """An affine problem: every inner iteration takes the full step, and the viol and J histories are those of al_cases.al_loop_lq run on the A, B the device
    returns, inside 32 max(e_ref, 2^-52) max|history| with e_ref the fp64-against-longdouble distance of the NumPy loop.

    The device linearizes as the reference does, with its regularised solve (REG = 1e-10 on the diagonal): the A, B it returns are the steps' own Jacobians
    [[1, h], [0, 1]] and [h^2, h] times m / (m + REG), 1e-10 below them, while its rollouts follow the steps (asserted here to the solver's tolerance and rounding).  The NumPy loop
    therefore takes the device's A, B where the device takes them -- in the backward pass -- and rolls out through the steps' map, as the device does.  With
    the device's A, B in the rollout as well the histories differ by 9e-10 (viol) and 5e-9 (J), which is that 1e-10 and nothing of the backward pass."""
    B, H, outer = 3, 8, 4
    RTOL = 1e-14                  # the steps are solved to this residual (a unit mass: a velocity), which bounds how closely a rollout follows the steps' map
    gm = api.BatchedMechanism(d.get_slider(timestep=0.05), B, dtype="f64", opts=d.SolverOptions(rtol=RTOL, btol=RTOL))
    try:
        x0 = T([[0.0, 0.0], [0.3, -0.5], [-0.4, 1.0]]); xg = np.array([0.5, 0.0])
        Q, R, Qf = 0.05 * np.eye(2), 0.01 * np.eye(1), np.eye(2)
        cost = ilqr.QuadraticCost(T(Q), T(R), T(Qf), T(xg))
        U0 = torch.zeros((H, B, 1), dtype=DT, device="cuda")
        res = ilqr.solve_constrained(gm, x0, U0, cost, ilqr.GoalConstraint(T(xg)), iters=1, outer=outer, act_off=0, na=1)
        X0, A, Bm, status = ilqr.linearize_rollout(gm, x0, U0)
        torch.cuda.synchronize()
        assert not status.any() and bool((res["a"] == 1.0).all()) and not res["fail"].any()
        assert res["viol"].shape == (outer + 1, B) and res["J"].shape == (outer + 1, B) and res["lam"].shape == (H + 1, B, 2) and res["rho"].shape == (B,)
        assert bool((res["rho"] == 1.0e4).all())
        present = np.zeros((H + 1, 2), bool); present[H] = True
        # the steps' map: a unit mass on a prismatic joint, v' = v + h (u + g), z' = z + h v'; the device's rollouts follow it to rounding, its A, B are 1e-10 off
        h = 0.05
        Ae, Be = np.array([[1.0, h], [0.0, 1.0]]), np.array([[h * h], [h]])
        An, Bn, X0n = A.cpu().numpy(), Bm.cpu().numpy(), X0.cpu().numpy()
        assert 0.5e-10 <= np.abs(Bn - Be).max() / h <= 2e-10 and np.abs(An - Ae).max() <= 2e-10
        c = X0n[1] - X0n[0] @ Ae.T                                                  # [B, 2]: the constant of the map, from the first step at u = 0
        for X, U in ((X0n, U0.cpu().numpy()), (res["X"].cpu().numpy(), res["U"].cpu().numpy())):
            defect = np.abs(X[1:] - (X[:-1] @ Ae.T + U @ Be.T + c)).max()
            print("slider: largest |X[k+1] - (Ae X[k] + Be U[k] + c)| = %.3e, max|X| %.3f" % (defect, np.abs(X).max()))
            assert defect <= RTOL + 64 * RC.U52 * np.abs(X).max()
        worst = 0.0
        roll = dict(A_roll=np.broadcast_to(Ae, (H, 2, 2)), B_roll=np.broadcast_to(Be, (H, 2, 1)))
        for b in range(B):
            args = (An[:, b], Bn[:, b], X0n[:, b], U0[:, b].cpu().numpy(), Q, R, Qf, xg, np.eye(2), xg, np.zeros(2, bool), present, outer)
            r64, rld = AC.al_loop_lq(*args, **roll), AC.al_loop_lq(*args, dtype=np.longdouble, **roll)
            for k in ("viol", "J"):
                ref = np.asarray(rld[k], np.float64); top = float(np.abs(ref).max())
                e_ref = float(np.abs(np.asarray(r64[k], np.float64) - ref).max()) / top
                err = float(np.abs(res[k][:, b].cpu().numpy() - ref).max()); unit = max(e_ref, RC.U52) * top
                print("slider env %d %s: |device - numpy| %.3e = %.2f units of max(e_ref, 2^-52) max|history| (e_ref %.2e); history %s" % (b, k, err, err / unit, e_ref, ref))
                worst = max(worst, err / unit)
            assert (np.diff(np.asarray(rld["viol"], np.float64)) < 0).all()           # the loop does contract the violation
        assert worst <= RC.FACTOR, worst
    finally:
        gm.close()


def cartpole(B, timestep=0.05):
    return api.BatchedMechanism(d.get_cartpole(timestep=timestep), B, dtype="f64", opts=d.SolverOptions(rtol=1e-8, btol=1e-8))


def cartpole_cost(ts):
    return ilqr.QuadraticCost(Q=T(np.diag([1.0, 0.1, 1.0, 0.1]) * ts), R=T(np.eye(1) * 0.01 * ts), Qf=T(np.diag([1.0, 0.1, 1.0, 0.1])), x_goal=torch.zeros(4, dtype=DT, device="cuda"))


def merit_never_rises(res, iters, outer):
    """per outer iteration: behind an accepted step the merit is below the one it started from, and the merit at the start of the next inner iteration (the same
    trajectory, rolled out again) is not above the start of this one, up to the rounding of two evaluations of one trajectory"""
    M, a = res["M"].cpu().numpy(), res["a"].cpu().numpy()
    assert M.shape == (iters * outer, 2, a.shape[1])
    acc = a > 0
    assert (M[:, 1][acc] <= M[:, 0][acc]).all()
    for o in range(outer):
        s = M[o * iters:(o + 1) * iters, 0]
        assert (s[1:] <= s[:-1] + 64 * RC.U52 * np.abs(s[:-1])).all(), s


def test_cartpole_reaches_its_goal_under_the_constraint():
    """four start angles, H = 30, a terminal goal with a modest Qf.  Measured on an MI355X: see DESIGN.md 5k."""
    B, H, iters, outer = 4, 30, 4, 5
    gm = cartpole(B)
    try:
        x0 = torch.zeros((B, 4), dtype=DT, device="cuda"); x0[:, 2] = torch.linspace(0.2, 0.8, B, dtype=DT, device="cuda")
        cost = cartpole_cost(0.05)
        U0 = torch.zeros((H, B, 2), dtype=DT, device="cuda")
        res = ilqr.solve_constrained(gm, x0, U0, cost, ilqr.GoalConstraint(torch.zeros(4, dtype=DT, device="cuda")), iters, outer, act_off=0, na=1)
        free = ilqr.solve(gm, x0, U0, cost, iters * outer, act_off=0, na=1)
        torch.cuda.synchronize()
        viol = res["viol"].cpu().numpy(); dist = free["X"][-1].abs().amax(1).cpu().numpy()
        print("cartpole viol per outer iteration:\n%s\nterminal distance of solve after %d iterations: %s\naccepted per iteration: %s" % (viol, iters * outer, dist, (res["a"] > 0).sum(1).tolist()))
        assert viol.shape == (outer + 1, B) and res["J"].shape == (iters * outer + 1, B) and np.isfinite(viol).all()
        assert np.array_equal(viol[-1], res["X"][-1].abs().amax(1).cpu().numpy())
        assert (viol[-1] < viol[1]).all(), viol
        assert (viol[-1] < dist).all(), (viol[-1], dist)
        merit_never_rises(res, iters, outer)
        ineq = torch.zeros(4, dtype=torch.bool)                                   # (a goal has no inequality rows: the statement is about none; StateBounds below has them)
        assert bool((res["lam"][:, :, ineq] >= 0).all())
        assert not res["U"][:, :, 1].any()                                          # the pole's input is not driven
        assert set(res) == set(free) | {"viol", "lam", "rho", "M"}
    finally:
        gm.close()


def test_state_bounds_on_the_cart_with_control_limits():
    """the cart may not leave |position| <= half of what the unconstrained swing reaches, under |u| <= F: every control inside the limits exactly, the multipliers
    of the inequality rows >= 0.  Measured on an MI355X: see DESIGN.md 5k."""
    B, H, iters, outer = 4, 30, 4, 5
    gm = cartpole(B)
    try:
        x0 = torch.zeros((B, 4), dtype=DT, device="cuda"); x0[:, 2] = torch.linspace(0.2, 0.8, B, dtype=DT, device="cuda")
        cost = cartpole_cost(0.05)
        U0 = torch.zeros((H, B, 2), dtype=DT, device="cuda")
        free = ilqr.solve(gm, x0, U0, cost, iters * outer, act_off=0, na=1)
        F = 0.75 * float(free["U"][:, :, 0].abs().max()); P = 0.5 * float(free["X"][:, :, 0].abs().max())
        assert F > 0 and P > 0
        bounds = ilqr.StateBounds(-P, P, rows=[0])
        res = ilqr.solve_constrained(gm, x0, U0, cost, bounds, iters, outer, lo=-F, hi=F, act_off=0, na=1)
        torch.cuda.synchronize()
        u = res["U"][:, :, 0].abs(); viol = res["viol"].cpu().numpy()
        print("state bounds |x_cart| <= %.4f (unconstrained: %.4f), |u| <= %.4f: largest |u| %.6f, %d of %d at the limit; bound violation per outer iteration:\n%s\nlargest |x_cart| %s" % (
            P, 2 * P, F, float(u.max()), int((u == F).sum()), u.numel(), viol, res["X"][:, :, 0].abs().amax(0).tolist()))
        assert bool((u <= F).all())
        assert res["lam"].shape == (H + 1, B, 2) and bool((res["lam"] >= 0).all()) and not res["lam"][0].any()
        assert "active" in res and res["active"].shape == (iters * outer, H, B)
        assert np.isfinite(viol).all() and (viol >= 0).all()
        merit_never_rises(res, iters, outer)
    finally:
        gm.close()


def test_no_constraint_rows_present_is_solve_limited():
    """a constraint object none of whose rows is present changes nothing: the bits of solve_limited (the backward pass then is dojo_riccati_box_dev's, bit for bit)"""
    B, H, iters = 3, 10, 3
    gm = cartpole(B)
    try:
        x0 = torch.zeros((B, 4), dtype=DT, device="cuda"); x0[:, 2] = torch.linspace(0.2, 0.6, B, dtype=DT, device="cuda")
        cost = cartpole_cost(0.05)
        U0 = torch.zeros((H, B, 2), dtype=DT, device="cuda")
        ref = ilqr.solve_limited(gm, x0, U0, cost, iters, -1.0, 1.0, act_off=0, na=1)
        res = ilqr.solve_constrained(gm, x0, U0, cost, ilqr.StateBounds(-np.inf, np.inf, rows=[0]), iters, 1, lo=-1.0, hi=1.0, act_off=0, na=1)
        for k in ref:
            assert torch.equal(ref[k], res[k]), k
        assert not res["viol"].any() and not res["lam"].any()
    finally:
        gm.close()


def test_example_runs_with_a_goal_at_a_small_batch():
    spec = importlib.util.spec_from_file_location("cartpole_ilqr_device", os.path.join(ROOT, "examples", "cartpole_ilqr_device.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    res = mod.main(["3", "20", "8", "--goal"])
    assert res["viol"].shape == (5, 3) and res["J"].shape == (9, 3) and bool(torch.isfinite(res["viol"]).all())
