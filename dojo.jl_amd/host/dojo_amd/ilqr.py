"""Batched iLQR in minimal coordinates (torch is plumbing only: it owns the buffers and evaluates the cost and the feedback law; the steps, their Jacobians and
the Riccati backward pass are the library's kernels).  The reference's examples/trajectory_optimization run IterativeLQR over get_minimal_gradients!; this is
the same loop for B environments at once -- one trajectory, one regularisation and one line search per environment, one launch per stage for the whole batch.

    X, A, Bm, status = linearize_rollout(gm, x0, U)                   # H calls of dojo_minimal_gradients_dev, writing into slices of A and Bm
    X, A, Bm, status = linearize_rollout_fused(gm, x0, U)             # the same as ONE call of dojo_rollout_minimal_dev, no join of the environment groups inside
    X, U, status = forward_pass_fused(gm, Xbar, Ubar, K, kff, a, ..)  # the closed-loop rollout around (Xbar, Ubar) for the step lengths a [B], ONE call
    K, kff, dV, fail = riccati(gm, A, Bm, lx, lu, lxx, luu)           # ONE launch of dojo_riccati_dev for all H steps
    res = solve(gm, x0, U0, QuadraticCost(Q, R, Qf, x_goal), iters=10)
    K, kff, dV, fail, active, qp_iters = riccati_box(gm, A, Bm, lx, lu, lxx, luu, U, lo, hi)   # ONE launch of dojo_riccati_box_dev: a box QP per step
    X, U, status = rollout_minimal_box(gm, x0, Ubar, lo, hi, Xbar, K, kff, a)                  # dojo_rollout_minimal_box_dev: the clamped tracking law
    res = solve_limited(gm, x0, U0, cost, 10, lo, hi)                                          # control-limited iLQR, lo <= u[act] <= hi
    K, kff, dV, fail, active, qp_iters = riccati_al(gm, A, Bm, lx, lu, lxx, luu, Cx, w, y)     # ONE launch of dojo_riccati_al_dev: the AL terms of constraint rows added in the kernel
    res = solve_constrained(gm, x0, U0, cost, GoalConstraint(x_goal), iters=4, outer=5)        # the augmented-Lagrangian loop: a terminal goal, state bounds
    Xt, Ut, st = rollout_minimal_fan(gm_trials, T, x0, Ubar, Xbar, K, kff, alpha, lo, hi)      # ONE call of dojo_rollout_minimal_fan_dev: T step lengths of P problems as T P environments
    sel = linesearch_select(gm_trials, T, Xt, Ut, st, alpha, dV, Xcur, Ucur, cost)             # ONE launch of dojo_linesearch_select_dev: costs, Armijo test, first accepted trial, gather
    res = solve_side_by_side(gm, gm_trials, x0, U0, cost, 10, lo, hi)                          # solve / solve_limited with the line search side by side, no read-back

Everything is enqueued on torch's current stream.  The drivers solve, solve_limited and solve_constrained read one flag per trial step length (have all
environments accepted?) and nothing else; solve_side_by_side reads nothing (include/dojo_hip_linesearch.h: it pays when an iteration needs two or more step lengths: DESIGN.md 5l has the measurements).
Not here (include/dojo_hip.h, "Batched iLQR"; include/dojo_hip_trajopt.h): costs shared across the batch, second-order dynamics terms, second-order constraint
terms and constraints evaluated on the device (control limits: include/dojo_hip_limits.h, solve_limited; other constraints: include/dojo_hip_constraints.h,
solve_constrained), constraints in the side-by-side driver, kinematic loops."""
import ctypes as C

import torch

from . import api


def _dtype(gm):
    return torch.float32 if gm.dtype_code == 1 else torch.float64


def _want(t, what, dt, shape):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != dt or tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be a %s device tensor of shape %s, got %s %s" % (what, dt, tuple(shape), t.dtype, tuple(t.shape)))
    return t.contiguous()


def linearize_rollout(gm, x0, U):
    """x0 [B,n] (n = 2 nu), U [H,B,nu] -> X [H+1,B,n] (X[0] = x0), A [H,B,n,n], Bm [H,B,n,nu], status [H,B] int32: H calls of dojo_minimal_gradients_dev, each
    stepping from X[k] into X[k+1] and writing its Jacobians straight into A[k], Bm[k] (row-major: the layout dojo_riccati_dev reads)."""
    B, nu = gm.batch, gm.spec.nu; n, dt = 2 * nu, _dtype(gm)
    if U.dim() != 3:
        raise ValueError("U must be [H, B, nu]")
    H = int(U.shape[0])
    U = _want(U, "U", dt, (H, B, nu)); x0 = _want(x0, "x0", dt, (B, n))
    dev = x0.device
    X = torch.empty((H + 1, B, n), dtype=dt, device=dev); X[0] = x0
    A = torch.empty((H, B, n, n), dtype=dt, device=dev); Bm = torch.empty((H, B, n, nu), dtype=dt, device=dev)
    status = torch.empty((H, B), dtype=torch.int32, device=dev); iters = torch.empty(B, dtype=torch.int32, device=dev)
    L, st = api.lib(), api.torch_stream(dev)
    for k in range(H):
        api._chk(L.dojo_minimal_gradients_dev(gm.h, api.addr(X[k]), api.addr(U[k]), api.addr(X[k + 1]), api.addr(status[k]), api.addr(iters), api.addr(A[k]), api.addr(Bm[k]), st))
    return X, A, Bm, status


def riccati(gm, A, Bm, lx, lu, lxx, luu, lux=None, mu=None, status=None, act_off=0, na=None, value=False):
    """dojo_riccati_dev on device tensors: A [H,B,n,n], Bm [H,B,n,nu], lx [H+1,B,n], lu [H,B,na], lxx [H+1,B,n,n], luu [H,B,na,na], lux [H,B,na,n] or None,
    mu [B] or None, status [H,B] int32 or None -> K [H,B,na,n], kff [H,B,na], dV [B,2], fail [B] int32 (and Vx [B,n], Vxx [B,n,n] with value).  One launch."""
    return _riccati(gm, A, Bm, lx, lu, lxx, luu, lux, mu, status, act_off, na, value, None)


def _riccati(gm, A, Bm, lx, lu, lxx, luu, lux, mu, status, act_off, na, value, _box, _con=None):
    """riccati (_box None), riccati_box (_box = (U, lo, hi)) and riccati_al (_con = (Cx, Cu, w, y, shared) on top): the checks and the outputs they share"""
    B, nu = gm.batch, gm.spec.nu; n, dt = 2 * nu, _dtype(gm)
    H = int(A.shape[0]); na = int(nu - act_off if na is None else na)
    A = _want(A, "A", dt, (H, B, n, n)); Bm = _want(Bm, "Bm", dt, (H, B, n, nu))
    lx = _want(lx, "lx", dt, (H + 1, B, n)); lu = _want(lu, "lu", dt, (H, B, na)); lxx = _want(lxx, "lxx", dt, (H + 1, B, n, n))
    luu = _want(luu, "luu", dt, (H, B, na, na)); lux = _want(lux, "lux", dt, (H, B, na, n)); mu = _want(mu, "mu", dt, (B,))
    status = _want(status, "status", torch.int32, (H, B))
    dev = A.device
    K = torch.empty((H, B, na, n), dtype=dt, device=dev); kff = torch.empty((H, B, na), dtype=dt, device=dev)
    dV = torch.empty((B, 2), dtype=dt, device=dev); fail = torch.empty(B, dtype=torch.int32, device=dev)
    Vx = torch.empty((B, n), dtype=dt, device=dev) if value else None; Vxx = torch.empty((B, n, n), dtype=dt, device=dev) if value else None
    r = api.DojoRiccati(*map(api.addr, (A, Bm, status, lx, lu, lxx, luu, lux, mu, K, kff, fail, dV, Vx, Vxx)), int(act_off), na)
    if _box is None:
        api._chk(api.lib().dojo_riccati_dev(gm.h, H, C.byref(r), api.torch_stream(dev)))
        return (K, kff, dV, fail, Vx, Vxx) if value else (K, kff, dV, fail)
    U, lo, hi = _box
    active = torch.empty((H, B), dtype=torch.int64, device=dev); qp_iters = torch.empty((H, B), dtype=torch.int32, device=dev)
    if _con is not None:
        Cx, Cu, w, y, shared = _con
        nc = 0 if w is None else int(w.shape[-1])
        Cx = _want(Cx, "Cx", dt, (nc, n) if shared else (H + 1, B, nc, n)); Cu = _want(Cu, "Cu", dt, (nc, na) if shared else (H, B, nc, na))
        w = _want(w, "w", dt, (H + 1, B, nc)); y = _want(y, "y", dt, (H + 1, B, nc))
        limited = lo is not None or hi is not None
        U = _want(U, "U", dt, (H, B, nu))
        if limited:
            lo, hi = _limits(gm, lo, hi, na, dev)
        lim = api.DojoControlLimits(api.addr(lo), api.addr(hi))
        con = api.DojoStageConstraints(api.addr(Cx), api.addr(Cu), api.addr(w), api.addr(y), nc, int(bool(shared)))
        api._chk(api.lib().dojo_riccati_al_dev(gm.h, H, C.byref(r), C.byref(lim) if limited else None, api.addr(U), C.byref(con), api.addr(active), api.addr(qp_iters),
                                               api.torch_stream(dev)))
        return (K, kff, dV, fail, active, qp_iters, Vx, Vxx) if value else (K, kff, dV, fail, active, qp_iters)
    U = _want(U, "U", dt, (H, B, nu)); lo, hi = _limits(gm, lo, hi, na, dev)
    lim = api.DojoControlLimits(api.addr(lo), api.addr(hi))
    api._chk(api.lib().dojo_riccati_box_dev(gm.h, H, C.byref(r), C.byref(lim), api.addr(U), api.addr(active), api.addr(qp_iters), api.torch_stream(dev)))
    return (K, kff, dV, fail, active, qp_iters, Vx, Vxx) if value else (K, kff, dV, fail, active, qp_iters)


def _limits(gm, lo, hi, na, dev):
    """lo, hi: a number, [na] or [B,na] (None: no limit on that side) -> two contiguous [B,na] device tensors in the handle dtype"""
    one = lambda v, none: torch.as_tensor(none if v is None else v, dtype=_dtype(gm), device=dev).expand(gm.batch, na).contiguous()
    return one(lo, float("-inf")), one(hi, float("inf"))


def riccati_box(gm, A, Bm, lx, lu, lxx, luu, U, lo, hi, lux=None, mu=None, status=None, act_off=0, na=None, value=False):
    """dojo_riccati_box_dev on device tensors: `riccati` under lo <= U[k][act] + kff[k] <= hi (a box QP per step, the gain rows of clamped inputs zero).  U [H,B,nu]:
    the controls the pass is taken around; lo, hi: [na] or [B,na] (a number or None also pass) -> K, kff, dV, fail (-(1 + k): the QP of step k failed or its box is
    empty), active [H,B] int64 (bit i: input act_off + i clamped), qp_iters [H,B] int32 (and Vx, Vxx with value).  One launch."""
    return _riccati(gm, A, Bm, lx, lu, lxx, luu, lux, mu, status, act_off, na, value, (U, lo, hi))


def riccati_al(gm, A, Bm, lx, lu, lxx, luu, Cx, w, y, Cu=None, shared=False, U=None, lo=None, hi=None, lux=None, mu=None, status=None, act_off=0, na=None,
               value=False):
    """dojo_riccati_al_dev on device tensors: `riccati_box` with the augmented-Lagrangian terms of nc linearized constraint rows per stage added inside the
    kernel -- G' diag(w) G to the step's Hessian, G' y to its gradient, G = [Cx Cu]; they never exist in memory.  Cx [H+1,B,nc,n], Cu [H,B,nc,na] or None
    (zeros), [nc,n] and [nc,na] with shared; w, y [H+1,B,nc]: the weight of a row (0: inactive or absent) and its multiplier estimate lambda + w c.  A row with
    w = y = 0 is not read.  lo, hi None: no control limits (U may then be None).  -> K, kff, dV, fail, active, qp_iters (and Vx, Vxx with value).  One launch."""
    return _riccati(gm, A, Bm, lx, lu, lxx, luu, lux, mu, status, act_off, na, value, (U, lo, hi), (Cx, Cu, w, y, shared))


class QuadraticCost:
    """J = sum_k 1/2 (x_k - g)' Q (x_k - g) + 1/2 u_k' R u_k  +  1/2 (x_H - g)' Qf (x_H - g) over the driven inputs u [na].  Q, Qf [n,n], R [na,na], x_goal [n]
    or [B,n]: device tensors in the handle's dtype.  Any object with `value` and `quadratize` can take its place in `solve`."""

    def __init__(self, Q, R, Qf, x_goal):
        self.Q, self.R, self.Qf, self.g = Q, R, Qf, x_goal

    def value(self, X, U):
        """X [H+1,B,n], U [H,B,na] -> J [B]"""
        d = X - self.g
        J = 0.5 * torch.einsum("kbi,ij,kbj->b", d[:-1], self.Q, d[:-1]) + 0.5 * torch.einsum("kbi,ij,kbj->b", U, self.R, U)
        return J + 0.5 * torch.einsum("bi,ij,bj->b", d[-1], self.Qf, d[-1])

    def quadratize(self, X, U):
        """-> lx [H+1,B,n], lu [H,B,na], lxx [H+1,B,n,n], luu [H,B,na,na], lux (None: zeros)"""
        H, B = U.shape[:2]
        d = X - self.g
        lx = torch.cat([d[:-1] @ self.Q.T, (d[-1] @ self.Qf.T)[None]], 0)
        lxx = torch.cat([self.Q.expand(H, B, -1, -1), self.Qf.expand(1, B, -1, -1)], 0).contiguous()
        return lx.contiguous(), (U @ self.R.T).contiguous(), lxx, self.R.expand(H, B, -1, -1).contiguous(), None


def forward_pass(gm, Xbar, Ubar, K, kff, a, act_off, na):
    """the closed-loop rollout for step length a: u_k[act] = Ubar_k[act] + a kff_k + K_k (x_k - Xbar_k) (torch), x_{k+1} by dojo_step_minimal_dev
    -> X [H+1,B,n], U [H,B,nu], status [H,B]"""
    H, B = Ubar.shape[:2]
    dev = Xbar.device
    X = torch.empty_like(Xbar); X[0] = Xbar[0]
    U = Ubar.clone()
    status = torch.empty((H, B), dtype=torch.int32, device=dev); iters = torch.empty(B, dtype=torch.int32, device=dev)
    L, st = api.lib(), api.torch_stream(dev)
    for k in range(H):
        U[k, :, act_off:act_off + na] += a * kff[k] + torch.einsum("bij,bj->bi", K[k], X[k] - Xbar[k])
        api._chk(L.dojo_step_minimal_dev(gm.h, api.addr(X[k]), api.addr(U[k]), api.addr(X[k + 1]), api.addr(status[k]), api.addr(iters), st))
    return X, U, status


def replay(gm, x0, U):
    """the open-loop rollout of U from x0 through dojo_step_minimal_dev -> X [H+1,B,n]"""
    H, B = U.shape[:2]
    X = torch.empty((H + 1, B, x0.shape[1]), dtype=x0.dtype, device=x0.device); X[0] = x0
    status = torch.empty(B, dtype=torch.int32, device=x0.device); iters = torch.empty(B, dtype=torch.int32, device=x0.device)
    L, st = api.lib(), api.torch_stream(x0.device)
    for k in range(H):
        api._chk(L.dojo_step_minimal_dev(gm.h, api.addr(X[k]), api.addr(U[k].contiguous()), api.addr(X[k + 1]), api.addr(status), api.addr(iters), st))
    return X


def rollout_minimal(gm, x0, Ubar, Xbar=None, K=None, kff=None, alpha=None, act_off=0, na=None, jacobians=False):
    """dojo_rollout_minimal_dev on device tensors: ONE call for the H steps from x0 [B,n] under u_k = Ubar[k] + E (alpha kff[k] + K[k] (x_k - Xbar[k])), every
    environment group at its own pace.  Ubar [H,B,nu], Xbar [H+1,B,n], K [H,B,na,n], kff [H,B,na] (riccati's outputs), alpha [B]; each of the last four may be None
    (zeros; alpha: ones).  -> X [H+1,B,n], U [H,B,nu], status [H,B] int32 and, with jacobians, A [H,B,n,n], Bm [H,B,n,nu]: what H calls of
    dojo_step_minimal_dev / dojo_minimal_gradients_dev at (X[k], U[k]) give, bit for bit."""
    return _rollout_minimal(gm, x0, Ubar, Xbar, K, kff, alpha, act_off, na, jacobians, None)


def _rollout_minimal(gm, x0, Ubar, Xbar, K, kff, alpha, act_off, na, jacobians, _box):
    """rollout_minimal (_box None) and rollout_minimal_box (_box = (lo, hi)): the checks and the outputs they share"""
    B, nu = gm.batch, gm.spec.nu; n, dt = 2 * nu, _dtype(gm)
    if Ubar.dim() != 3:
        raise ValueError("Ubar must be [H, B, nu]")
    H = int(Ubar.shape[0]); na = int(nu - act_off if na is None else na)
    x0 = _want(x0, "x0", dt, (B, n)); Ubar = _want(Ubar, "Ubar", dt, (H, B, nu)); Xbar = _want(Xbar, "Xbar", dt, (H + 1, B, n))
    K = _want(K, "K", dt, (H, B, na, n)); kff = _want(kff, "kff", dt, (H, B, na)); alpha = _want(alpha, "alpha", dt, (B,))
    dev = x0.device
    X = torch.empty((H + 1, B, n), dtype=dt, device=dev); U = torch.empty((H, B, nu), dtype=dt, device=dev)
    status = torch.empty((H, B), dtype=torch.int32, device=dev)
    A = torch.empty((H, B, n, n), dtype=dt, device=dev) if jacobians else None; Bm = torch.empty((H, B, n, nu), dtype=dt, device=dev) if jacobians else None
    t = api.DojoTracking(*map(api.addr, (x0, Ubar, Xbar, K, kff, alpha, X, U, status, A, Bm)), int(act_off), na)
    if _box is None:
        api._chk(api.lib().dojo_rollout_minimal_dev(gm.h, H, C.byref(t), api.torch_stream(dev)))
    else:
        lo, hi = _limits(gm, _box[0], _box[1], na, dev)
        lim = api.DojoControlLimits(api.addr(lo), api.addr(hi))
        api._chk(api.lib().dojo_rollout_minimal_box_dev(gm.h, H, C.byref(t), C.byref(lim), api.torch_stream(dev)))
    return (X, U, status, A, Bm) if jacobians else (X, U, status)


def rollout_minimal_box(gm, x0, Ubar, lo, hi, Xbar=None, K=None, kff=None, alpha=None, act_off=0, na=None, jacobians=False):
    """dojo_rollout_minimal_box_dev on device tensors: `rollout_minimal` with the driven inputs clamped into [lo, hi] ([na] or [B,na]; a number or None also pass)
    in fp64 before they are rounded and stepped.  With infinite limits: rollout_minimal's outputs, bit for bit."""
    return _rollout_minimal(gm, x0, Ubar, Xbar, K, kff, alpha, act_off, na, jacobians, (lo, hi))


def forward_pass_box(gm, Xbar, Ubar, K, kff, a, act_off, na, lo, hi):
    """forward_pass with the driven inputs clamped into [lo, hi] (torch.clamp) -> X [H+1,B,n], U [H,B,nu], status [H,B]"""
    H, B = Ubar.shape[:2]
    dev = Xbar.device
    lo, hi = _limits(gm, lo, hi, na, dev)
    X = torch.empty_like(Xbar); X[0] = Xbar[0]
    U = Ubar.clone()
    status = torch.empty((H, B), dtype=torch.int32, device=dev); iters = torch.empty(B, dtype=torch.int32, device=dev)
    L, st = api.lib(), api.torch_stream(dev)
    for k in range(H):
        U[k, :, act_off:act_off + na] += a * kff[k] + torch.einsum("bij,bj->bi", K[k], X[k] - Xbar[k])
        U[k, :, act_off:act_off + na] = torch.clamp(U[k, :, act_off:act_off + na], lo, hi)
        api._chk(L.dojo_step_minimal_dev(gm.h, api.addr(X[k]), api.addr(U[k]), api.addr(X[k + 1]), api.addr(status[k]), api.addr(iters), st))
    return X, U, status


def forward_pass_fused_box(gm, Xbar, Ubar, K, kff, alpha, act_off, na, lo, hi):
    """forward_pass_box as one call of dojo_rollout_minimal_box_dev, the law and the clamp evaluated on the device in fp64"""
    if not torch.is_tensor(alpha):
        alpha = torch.full((gm.batch,), float(alpha), dtype=_dtype(gm), device=Xbar.device)
    return rollout_minimal_box(gm, Xbar[0].contiguous(), Ubar, lo, hi, Xbar, K, kff, alpha, act_off, na)


def linearize_rollout_fused(gm, x0, U):
    """linearize_rollout as one call of dojo_rollout_minimal_dev: the same X, A, Bm, status, bit for bit"""
    X, _, status, A, Bm = rollout_minimal(gm, x0, U, na=1, jacobians=True)
    return X, A, Bm, status


def forward_pass_fused(gm, Xbar, Ubar, K, kff, alpha, act_off, na):
    """forward_pass as one call of dojo_rollout_minimal_dev, the feedback law evaluated on the device in fp64; alpha: a float or a [B] tensor (one step length per
    environment) -> X [H+1,B,n], U [H,B,nu], status [H,B]"""
    if not torch.is_tensor(alpha):
        alpha = torch.full((gm.batch,), float(alpha), dtype=_dtype(gm), device=Xbar.device)
    return rollout_minimal(gm, Xbar[0].contiguous(), Ubar, Xbar, K, kff, alpha, act_off, na)


def solve(gm, x0, U0, cost, iters, act_off=0, na=None, c1=1e-4, alphas=(1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125),
          mu_init=0.0, mu_min=1e-6, mu_grow=10.0, mu_shrink=0.1, fused=False):
    """iLQR for B environments.  x0 [B,n], U0 [H,B,nu] (all inputs; the policy drives act_off .. act_off + na - 1, na = nu - act_off by default, the others keep
    U0's values), cost: an object with value(X, U_act) -> J [B] and quadratize(X, U_act) -> (lx, lu, lxx, luu, lux).  Each of the `iters` iterations:
      1. linearize_rollout along the current controls: X, A, Bm, status;  J_old = cost.value
      2. cost.quadratize, riccati with the per-environment regularisation mu -> K, kff, dV, fail
      3. for a in alphas (defaults: 1, 1/2, .. 1/128), the whole batch at once: forward_pass; environment b ACCEPTS the first a with
             J_new <= J_old + c1 (a dV[0] + a^2 dV[1])     (c1 = 1e-4; dV[0] < 0: an Armijo condition on the model's expected change)
         and no failed step in either rollout and fail[b] = 0 (torch.where per environment); the trials stop once every environment has accepted
      4. mu: an environment that accepted: mu <- mu_shrink mu (0.1), set to 0 below mu_min (1e-6); one with fail != 0 or without an accepted a:
         mu <- max(mu_grow mu, mu_min) (x 10) and its controls stay as they were.  mu starts as mu_init (0).
    -> dict: X [H+1,B,n], U [H,B,nu] (the last accepted trajectory of every environment), J [iters+1,B] (J[i]: the cost at the start of iteration i, J[iters]:
    at the end), a [iters,B] (the accepted step length, 0: none), mu [iters,B] (the regularisation each backward pass ran with), fail [iters,B], dV [iters,B,2].
    fused: steps 1 and 3 are one call of dojo_rollout_minimal_dev each (linearize_rollout_fused, forward_pass_fused) instead of H calls driven from here."""
    return _solve(gm, x0, U0, cost, iters, act_off, na, c1, alphas, mu_init, mu_min, mu_grow, mu_shrink, fused, None)


def solve_limited(gm, x0, U0, cost, iters, lo, hi, act_off=0, na=None, c1=1e-4, alphas=(1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125),
                  mu_init=0.0, mu_min=1e-6, mu_grow=10.0, mu_shrink=0.1, fused=False):
    """control-limited iLQR (Tassa, Mansard, Todorov, ICRA 2014): `solve` under lo <= u[act] <= hi at every step, lo and hi [na] or [B,na] (+-inf allowed).
    U0[:, :, act] is clamped into the limits first; the backward pass is riccati_box (a box QP per step around the current controls, the gain rows of clamped
    inputs zero), the forward pass clamps (forward_pass_box; fused: one call of dojo_rollout_minimal_box_dev).  Everything else, the acceptance test included, is
    `solve`'s.  -> solve's dict and active [iters,H,B] int64 (bit i: input act_off + i clamped in that backward pass).  With infinite limits: solve's bits."""
    return _solve(gm, x0, U0, cost, iters, act_off, na, c1, alphas, mu_init, mu_min, mu_grow, mu_shrink, fused, (lo, hi))


def _solve(gm, x0, U0, cost, iters, act_off, na, c1, alphas, mu_init, mu_min, mu_grow, mu_shrink, fused, limits, al=None):
    """the loop of solve (limits None) and solve_limited (limits = (lo, hi)).  al (solve_constrained's _AugmentedLagrangian, None for the two others, whose
    statements are then exactly what they were): the backward pass is riccati_al over al.terms, and the merit M = J + al.penalty takes J's place in the
    acceptance test; the regularisation starts from al.mu and is left there"""
    B, nu = gm.batch, gm.spec.nu; dt = _dtype(gm)
    na = int(nu - act_off if na is None else na)
    dev = x0.device
    U = U0.clone()
    mu = torch.full((B,), float(mu_init), dtype=dt, device=dev)
    hist = {"J": [], "a": [], "mu": [], "fail": [], "dV": []}
    act = slice(act_off, act_off + na)
    if limits is not None:
        lo, hi = _limits(gm, limits[0], limits[1], na, dev)
        U[:, :, act] = torch.clamp(U[:, :, act], lo, hi)
        hist["active"] = []
    if al is not None:
        hist["M"] = []
        if al.mu is not None:
            mu = al.mu
    if int(iters) < 1:
        raise ValueError("iters must be >= 1")
    for _ in range(int(iters)):
        X, A, Bm, status = (linearize_rollout_fused if fused else linearize_rollout)(gm, x0, U)
        J = cost.value(X, U[:, :, act])
        lx, lu, lxx, luu, lux = cost.quadratize(X, U[:, :, act])
        if al is not None:
            Cx, Cu, shared, w, y, pen = al.terms(X, U[:, :, act])
            M = M_acc = J + pen
            K, kff, dV, fail, active, _ = riccati_al(gm, A, Bm, lx, lu, lxx, luu, Cx, w, y, Cu, shared, U if limits is not None else None,
                                                     lo if limits is not None else None, hi if limits is not None else None, lux, mu, status, act_off, na)
            if limits is not None:
                hist["active"].append(active)
        elif limits is None:
            K, kff, dV, fail = riccati(gm, A, Bm, lx, lu, lxx, luu, lux, mu, status, act_off, na)
        else:
            K, kff, dV, fail, active, _ = riccati_box(gm, A, Bm, lx, lu, lxx, luu, U, lo, hi, lux, mu, status, act_off, na)
            hist["active"].append(active)
        solved = (status == 0).all(0) & (fail == 0)
        accepted = torch.zeros(B, dtype=torch.bool, device=dev)
        a_acc = torch.zeros(B, dtype=dt, device=dev)
        U_new = U.clone()
        for a in alphas:
            if limits is None:
                Xa, Ua, sa = (forward_pass_fused if fused else forward_pass)(gm, X, U, K, kff, float(a), act_off, na)
            else:
                Xa, Ua, sa = (forward_pass_fused_box if fused else forward_pass_box)(gm, X, U, K, kff, float(a), act_off, na, lo, hi)
            Ja = cost.value(Xa, Ua[:, :, act])
            if al is None:
                now = ~accepted & solved & (sa == 0).all(0) & (Ja <= J + c1 * (a * dV[:, 0] + a * a * dV[:, 1]))
            else:
                Ma = Ja + al.penalty(Xa, Ua[:, :, act])
                now = ~accepted & solved & (sa == 0).all(0) & (Ma <= M + c1 * (a * dV[:, 0] + a * a * dV[:, 1]))
                M_acc = torch.where(now, Ma, M_acc)
            U_new = torch.where(now[None, :, None], Ua, U_new); a_acc = torch.where(now, torch.full_like(a_acc, a), a_acc)
            accepted |= now
            if bool((accepted | ~solved).all()):
                break
        hist["J"].append(J); hist["a"].append(a_acc); hist["mu"].append(mu.clone()); hist["fail"].append(fail); hist["dV"].append(dV)
        shrunk = mu * mu_shrink
        mu = torch.where(accepted, torch.where(shrunk < mu_min, torch.zeros_like(mu), shrunk), torch.clamp(mu * mu_grow, min=mu_min))
        U = U_new
        if al is not None:
            hist["M"].append(torch.stack([M, M_acc]))
    if al is not None:
        al.mu = mu
    X = replay(gm, x0, U)
    hist["J"].append(cost.value(X, U[:, :, act]))
    return {"X": X, "U": U, **{k: torch.stack(v) for k, v in hist.items()}}


# ---- the line search side by side (include/dojo_hip_linesearch.h): T step lengths of P problems as ONE rollout of T P environments, ONE selection kernel ----
def rollout_minimal_fan(gm_trials, T, x0, Ubar, Xbar, K, kff, alpha, lo=None, hi=None, act_off=0, na=None):
    """dojo_rollout_minimal_fan_dev on device tensors.  gm_trials: a handle of batch T P; environment tr P + p is trial tr of problem p.  x0 [P,n], Ubar [H,P,nu],
    Xbar [H+1,P,n], K [H,P,na,n], kff [H,P,na] (Xbar, K, kff may be None) and lo, hi ([na] or [P,na], a number or None; both None: no limits) are per problem and
    are read at e mod P; alpha [T,P] is per environment.  -> X [H+1,T P,n], U [H,T P,nu], status [H,T P] int32: rollout_minimal_box's (rollout_minimal's without
    limits) on the inputs repeated T times, bit for bit."""
    B, nu, T = gm_trials.batch, gm_trials.spec.nu, int(T); n, dt = 2 * nu, _dtype(gm_trials)
    if T < 1 or B % T:
        raise ValueError("the batch of gm_trials (%d) must be T (%d) trials of P problems" % (B, T))
    if Ubar.dim() != 3:
        raise ValueError("Ubar must be [H, P, nu]")
    P, H = B // T, int(Ubar.shape[0]); na = int(nu - act_off if na is None else na)
    x0 = _want(x0, "x0", dt, (P, n)); Ubar = _want(Ubar, "Ubar", dt, (H, P, nu)); Xbar = _want(Xbar, "Xbar", dt, (H + 1, P, n))
    K = _want(K, "K", dt, (H, P, na, n)); kff = _want(kff, "kff", dt, (H, P, na)); alpha = _want(alpha, "alpha", dt, (T, P))
    dev = x0.device
    X = torch.empty((H + 1, B, n), dtype=dt, device=dev); U = torch.empty((H, B, nu), dtype=dt, device=dev)
    status = torch.empty((H, B), dtype=torch.int32, device=dev)
    t = api.DojoTracking(*map(api.addr, (x0, Ubar, Xbar, K, kff, alpha, X, U, status, None, None)), int(act_off), na)
    limited = lo is not None or hi is not None
    if limited:
        one = lambda v, none: torch.as_tensor(none if v is None else v, dtype=dt, device=dev).expand(P, na).contiguous()
        lo, hi = one(lo, float("-inf")), one(hi, float("inf"))
    lim = api.DojoControlLimits(api.addr(lo), api.addr(hi))
    api._chk(api.lib().dojo_rollout_minimal_fan_dev(gm_trials.h, H, T, C.byref(t), C.byref(lim) if limited else None, api.torch_stream(dev)))
    return X, U, status


def linesearch_select(gm_trials, T, X, U, status, alpha, dV, Xcur, Ucur, cost=None, ok=None, J0=None, J_trial=None, c1=1e-4, act_off=0, na=None, gather=True):
    """dojo_linesearch_select_dev on device tensors: of the T trials X [H+1,T P,n], U [H,T P,nu], status [H,T P] (None: all solved) of every problem the FIRST with
    ok[p] != 0 (ok [P] int32 or None), no failed step and J_tr <= J0 + c1 (a dV[p,0] + a^2 dV[p,1]), a = alpha[tr,p].  cost: a QuadraticCost -- the costs are
    evaluated in the kernel in fp64 (J0 too, from Xcur [H+1,P,n], Ucur [H,P,nu], unless given); None: J_trial [T,P] and J0 [P] (float64) are the caller's (any
    cost object, the merit of an augmented Lagrangian).  -> dict: choice [P] int32 (-1: none), alpha [P] (0: none), J_trial [T,P], J_cur [P], J_acc [P] (float64)
    and, with gather, X [H+1,P,n], U [H,P,nu]: exact copies of the accepted trial's columns, or of Xcur, Ucur.  One launch, nothing is read back."""
    B, nu, T = gm_trials.batch, gm_trials.spec.nu, int(T); n, dt = 2 * nu, _dtype(gm_trials)
    if T < 1 or B % T:
        raise ValueError("the batch of gm_trials (%d) must be T (%d) trials of P problems" % (B, T))
    P, H = B // T, int(U.shape[0]); na = int(nu - act_off if na is None else na)
    X = _want(X, "X", dt, (H + 1, B, n)); U = _want(U, "U", dt, (H, B, nu)); status = _want(status, "status", torch.int32, (H, B))
    alpha = _want(alpha, "alpha", dt, (T, P)); dV = _want(dV, "dV", dt, (P, 2)); ok = _want(ok, "ok", torch.int32, (P,))
    Xcur = _want(Xcur, "Xcur", dt, (H + 1, P, n)); Ucur = _want(Ucur, "Ucur", dt, (H, P, nu)); J0 = _want(J0, "J0", torch.float64, (P,))
    dev = X.device
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    J_trial = f64(T, P) if cost is not None else _want(J_trial, "J_trial", torch.float64, (T, P))
    J_cur, J_acc = f64(P), f64(P)
    choice = torch.empty(P, dtype=torch.int32, device=dev); a_acc = torch.empty(P, dtype=dt, device=dev)
    Xn = torch.empty((H + 1, P, n), dtype=dt, device=dev) if gather else None; Un = torch.empty((H, P, nu), dtype=dt, device=dev) if gather else None
    qc = None
    if cost is not None:
        per = cost.g.dim() == 2
        keep = (_want(cost.Q, "Q", dt, (n, n)), _want(cost.R, "R", dt, (na, na)), _want(cost.Qf, "Qf", dt, (n, n)), _want(cost.g, "x_goal", dt, (P, n) if per else (n,)))
        qc = api.DojoQuadraticCost(*map(api.addr, keep), int(per))
    ls = api.DojoLineSearch(*map(api.addr, (X, U, status, alpha, dV, ok, Xcur, Ucur, J0, J_trial, J_cur, J_acc, choice, a_acc, Xn, Un)), float(c1), int(act_off), na)
    api._chk(api.lib().dojo_linesearch_select_dev(gm_trials.h, H, T, None if qc is None else C.byref(qc), C.byref(ls), api.torch_stream(dev)))
    out = {"choice": choice, "alpha": a_acc, "J_trial": J_trial, "J_cur": J_cur, "J_acc": J_acc}
    if gather:
        out.update(X=Xn, U=Un)
    return out


def solve_side_by_side(gm, gm_trials, x0, U0, cost, iters, lo=None, hi=None, act_off=0, na=None, c1=1e-4,
                       alphas=(1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125), mu_init=0.0, mu_min=1e-6, mu_grow=10.0, mu_shrink=0.1):
    """`solve` (lo and hi None) / `solve_limited` with the step lengths of the line search side by side.  gm: a handle of batch P for the linearization and the
    backward pass; gm_trials: a handle of the same mechanism and dtype with batch len(alphas) P for the trials; alphas: numbers, or a device tensor [T] or [T,P] (a
    ladder per problem).  Each iteration:
      1. linearize_rollout on gm;  2. cost.quadratize;  3. riccati (riccati_box with limits) on gm;
      4. ONE fan rollout of all step lengths on gm_trials (rollout_minimal_fan);
      5. ONE selection (linesearch_select): a QuadraticCost is evaluated by the kernel in fp64, any other cost object by cost.value on the [H+1,T P,n] trials and
         handed over as J_trial; the first acceptable step length of every problem wins, as in `solve`;
      6. `solve`'s update of mu from choice >= 0 (torch.where).
    The loop reads nothing back from the device: all of it is enqueued on torch's current stream.
    -> solve's dict (J, and the decisions, are fp64 whatever the handle dtype) plus choice [iters,P] int32 and J_trial [iters,T,P]; with limits also active."""
    P, nu = gm.batch, gm.spec.nu; dt = _dtype(gm)
    T = int(alphas.shape[0]) if torch.is_tensor(alphas) else len(alphas)
    if gm_trials.batch != T * P or gm_trials.dtype_code != gm.dtype_code:
        raise ValueError("gm_trials must have batch len(alphas) * gm.batch = %d and gm's dtype" % (T * P))
    if int(iters) < 1:
        raise ValueError("iters must be >= 1")
    na = int(nu - act_off if na is None else na)
    dev = x0.device
    act = slice(act_off, act_off + na)
    U = U0.clone()
    limited = lo is not None or hi is not None
    hist = {"J": [], "a": [], "mu": [], "fail": [], "dV": [], "choice": [], "J_trial": []}
    if limited:
        lo, hi = _limits(gm, lo, hi, na, dev)
        U[:, :, act] = torch.clamp(U[:, :, act], lo, hi)
        hist["active"] = []
    mu = torch.full((P,), float(mu_init), dtype=dt, device=dev)
    if torch.is_tensor(alphas):          # [T] or [T,P] on the device: nothing is uploaded
        alpha = _want(alphas if alphas.dim() == 2 else alphas[:, None].expand(T, P), "alphas", dt, (T, P))
    else:
        alpha = torch.tensor([float(a) for a in alphas], dtype=dt, device=dev)[:, None].expand(T, P).contiguous()
    device_cost = isinstance(cost, QuadraticCost)
    for _ in range(int(iters)):
        X, A, Bm, status = linearize_rollout(gm, x0, U)
        lx, lu, lxx, luu, lux = cost.quadratize(X, U[:, :, act])
        if limited:
            K, kff, dV, fail, active, _ = riccati_box(gm, A, Bm, lx, lu, lxx, luu, U, lo, hi, lux, mu, status, act_off, na)
            hist["active"].append(active)
        else:
            K, kff, dV, fail = riccati(gm, A, Bm, lx, lu, lxx, luu, lux, mu, status, act_off, na)
        ok = ((status == 0).all(0) & (fail == 0)).to(torch.int32)
        Xt, Ut, st = rollout_minimal_fan(gm_trials, T, x0, U, X, K, kff, alpha, lo if limited else None, hi if limited else None, act_off, na)
        if device_cost:
            sel = linesearch_select(gm_trials, T, Xt, Ut, st, alpha, dV, X, U, cost, ok, None, None, c1, act_off, na)
        else:
            J0 = cost.value(X, U[:, :, act]).to(torch.float64)
            Jt = cost.value(Xt, Ut[:, :, act]).to(torch.float64).view(T, P).contiguous()
            sel = linesearch_select(gm_trials, T, Xt, Ut, st, alpha, dV, X, U, None, ok, J0, Jt, c1, act_off, na)
        accepted = sel["choice"] >= 0
        hist["J"].append(sel["J_cur"]); hist["a"].append(sel["alpha"]); hist["mu"].append(mu.clone()); hist["fail"].append(fail); hist["dV"].append(dV)
        hist["choice"].append(sel["choice"]); hist["J_trial"].append(sel["J_trial"])
        shrunk = mu * mu_shrink
        mu = torch.where(accepted, torch.where(shrunk < mu_min, torch.zeros_like(mu), shrunk), torch.clamp(mu * mu_grow, min=mu_min))
        U = sel["U"]
    X = replay(gm, x0, U)
    hist["J"].append(cost.value(X, U[:, :, act]).to(torch.float64))
    return {"X": X, "U": U, **{k: torch.stack(v) for k, v in hist.items()}}


# ---- constraints other than control limits: the augmented-Lagrangian loop of IterativeLQR around the iLQR above (include/dojo_hip_constraints.h) ----
class GoalConstraint:
    """the terminal equality x_H[rows] = x_goal[rows] (rows: indices into the n state coordinates, default all): c = x_H[rows] - x_goal[rows] at stage H, absent at
    the stages before.  x_goal [n] or [B,n], a device tensor in the handle's dtype.  The Jacobian is shared by the stages and the batch."""

    def __init__(self, x_goal, rows=None):
        n = int(x_goal.shape[-1])
        self.rows = torch.arange(n, device=x_goal.device) if rows is None else torch.as_tensor(rows, dtype=torch.long, device=x_goal.device)
        self.goal, self.n, self.nc = x_goal, n, int(self.rows.numel())
        self.ineq = torch.zeros(self.nc, dtype=torch.bool, device=x_goal.device)
        self._Cx = torch.zeros((self.nc, n), dtype=x_goal.dtype, device=x_goal.device)
        self._Cx[torch.arange(self.nc, device=x_goal.device), self.rows] = 1.0

    def present(self, H):
        p = torch.zeros((H + 1, self.nc), dtype=torch.bool, device=self.goal.device); p[H] = True
        return p

    def evaluate(self, X, U_act):
        return (X - self.goal)[..., self.rows]

    def jacobians(self, X, U_act):
        return self._Cx, None, True


class StateBounds:
    """lo <= x_k[rows] <= hi at the stages k = 1 .. H as 2 len(rows) inequalities c <= 0: c = [x[rows] - hi; lo - x[rows]] (rows: indices into the n state
    coordinates, default all).  lo, hi: numbers or [len(rows)] (+-inf: no bound on that side; its row is absent).  The Jacobian is shared by the stages and the batch."""

    def __init__(self, lo, hi, rows=None):
        self._lo, self._hi, self._rows, self._built = lo, hi, rows, None
        r = len(rows) if rows is not None else max(int(torch.as_tensor(v).numel()) for v in (lo, hi))
        if rows is None and r == 1:
            raise ValueError("StateBounds: with scalar bounds give the rows they apply to")
        self.nc = 2 * r

    def _build(self, X):
        """the tensors, on X's device in X's dtype, at the first use"""
        if self._built is None or self._built != (X.dtype, X.device):
            dt, dev, r, n = X.dtype, X.device, self.nc // 2, int(X.shape[-1])
            self.rows = torch.arange(n, device=dev) if self._rows is None else torch.as_tensor(self._rows, dtype=torch.long, device=dev)
            self.lo = torch.as_tensor(self._lo, dtype=dt, device=dev).expand(r).contiguous(); self.hi = torch.as_tensor(self._hi, dtype=dt, device=dev).expand(r).contiguous()
            self.Cx = torch.zeros((self.nc, n), dtype=dt, device=dev)
            i = torch.arange(r, device=dev)
            self.Cx[i, self.rows] = 1.0; self.Cx[r + i, self.rows] = -1.0
            self._built = (dt, dev)

    @property
    def ineq(self):
        return torch.ones(self.nc, dtype=torch.bool)

    def present(self, H):
        finite = torch.isfinite(torch.cat([torch.as_tensor(self._hi, dtype=torch.float64).expand(self.nc // 2), torch.as_tensor(self._lo, dtype=torch.float64).expand(self.nc // 2)]).cpu())
        p = finite[None].repeat(H + 1, 1); p[0] = False
        return p

    def evaluate(self, X, U_act):
        self._build(X)
        x = X[..., self.rows]
        c = torch.cat([x - self.hi, self.lo - x], -1)
        return torch.where(torch.isfinite(c), c, torch.full_like(c, -1.0))         # (an infinite bound: its row is absent, any finite value does)

    def jacobians(self, X, U_act):
        self._build(X)
        return self.Cx, None, True


class _AugmentedLagrangian:
    """what _solve needs of the outer loop's state: the multipliers lam [H+1,B,nc], the penalty rho [B], the regularisation carried across the outer iterations"""

    def __init__(self, con, H, B, rho0, dt, dev):
        present = con.present(H) if callable(con.present) else con.present           # [H+1,nc] bool: a tensor, or a function of the horizon
        self.con, self.present, self.ineq = con, torch.as_tensor(present, device=dev)[:, None, :], torch.as_tensor(con.ineq, device=dev)[None, None, :]
        self.lam = torch.zeros((H + 1, B, con.nc), dtype=dt, device=dev); self.rho = torch.full((B,), float(rho0), dtype=dt, device=dev)
        self.mu = None

    def weights(self, c):
        """a = present & (~ineq | c >= 0 | lam > 0), w = rho a, y = lam + w c"""
        a = self.present & (~self.ineq | (c >= 0) | (self.lam > 0))
        w = self.rho[None, :, None] * a
        return w, self.lam + w * c

    def penalty(self, X, U_act):
        """sum lam c + 1/2 sum w c^2 -> [B]"""
        c = self.con.evaluate(X, U_act) * self.present
        w, _ = self.weights(c)
        return (self.lam * c).sum((0, 2)) + 0.5 * (w * c * c).sum((0, 2))

    def terms(self, X, U_act):
        c = self.con.evaluate(X, U_act) * self.present
        w, y = self.weights(c)
        Cx, Cu, shared = self.con.jacobians(X, U_act)
        return Cx, Cu, shared, w.contiguous(), y.contiguous(), (self.lam * c).sum((0, 2)) + 0.5 * (w * c * c).sum((0, 2))

    def violation(self, X, U_act):
        c = self.con.evaluate(X, U_act)
        v = torch.where(self.ineq, torch.clamp(c, min=0.0), c.abs()) * self.present
        return v.amax((0, 2)), c

    def update(self, c, rho_scale, rho_max):
        """lam <- lam + rho c (equalities), max(0, lam + rho c) (inequalities) on the present rows; rho <- min(rho_scale rho, rho_max)"""
        new = self.lam + self.rho[None, :, None] * c
        self.lam = torch.where(self.present, torch.where(self.ineq, torch.clamp(new, min=0.0), new), self.lam)
        self.rho = torch.clamp(self.rho * rho_scale, max=rho_max)


def solve_constrained(gm, x0, U0, cost, constraints, iters, outer, lo=None, hi=None, rho0=1.0, rho_scale=10.0, rho_max=1e8, act_off=0, na=None, c1=1e-4,
                      alphas=(1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125), mu_init=0.0, mu_min=1e-6, mu_grow=10.0, mu_shrink=0.1, fused=False):
    """iLQR under constraints c(x, u) = 0 / <= 0 by IterativeLQR's augmented-Lagrangian loop.  `constraints`: an object with nc, ineq [nc] bool (the convention is
    c <= 0), present [H+1,nc] bool (or a function of H that gives it), evaluate(X, U_act) -> c [H+1,B,nc] and jacobians(X, U_act) -> (Cx, Cu or None, shared) in riccati_al's layouts
    (GoalConstraint, StateBounds).  lo, hi: control limits as in solve_limited -- they go to the box QP of the backward pass and the clamp of the forward pass, not
    into the augmented Lagrangian.  With lam = 0 and rho [B] = rho0 at the start, each of the `outer` iterations runs
      * `iters` iterations of `solve` with the merit  M = J + sum lam c + 1/2 sum w c^2  in J's place in the acceptance test and riccati_al as the backward pass,
        where, from the current c, before every backward pass and every evaluation of M:  a = present & (~ineq | c >= 0 | lam > 0),  w = rho a,  y = lam + w c
        (the kernel's dV is the model of exactly this M);
      * then, on the present rows:  lam <- lam + rho c  (equalities),  lam <- max(0, lam + rho c)  (inequalities);  rho <- min(rho_scale rho, rho_max).
    The regularisation mu carries over from one outer iteration to the next.
    -> solve's dict over all outer x iters iterations (J [outer iters + 1,B] is the cost alone; M [outer iters,2,B]: the merit at the start of an iteration and behind
    its accepted step), viol [outer+1,B] (the largest |c| of an equality, max(c, 0) of an inequality over the present rows, before the first and behind every outer
    iteration), lam [H+1,B,nc], rho [B]."""
    B, nu = gm.batch, gm.spec.nu; dt = _dtype(gm)
    na = int(nu - act_off if na is None else na)
    H, dev = int(U0.shape[0]), x0.device
    act = slice(act_off, act_off + na)
    if int(outer) < 1:
        raise ValueError("outer must be >= 1")
    limits = None if lo is None and hi is None else (lo, hi)
    al = _AugmentedLagrangian(constraints, H, B, rho0, dt, dev)
    U = U0.clone()
    if limits is not None:
        l, h = _limits(gm, lo, hi, na, dev)
        U[:, :, act] = torch.clamp(U[:, :, act], l, h)
    viol = [al.violation(replay(gm, x0, U), U[:, :, act])[0]]
    parts = []
    for _ in range(int(outer)):
        res = _solve(gm, x0, U, cost, iters, act_off, na, c1, alphas, mu_init, mu_min, mu_grow, mu_shrink, fused, limits, al)
        U = res["U"]
        v, c = al.violation(res["X"], U[:, :, act])
        viol.append(v)
        al.update(c * al.present, rho_scale, rho_max)
        parts.append(res)
    out = {"X": parts[-1]["X"], "U": U}
    for k in parts[0]:
        if k == "J":
            out[k] = torch.cat([p[k][:-1] for p in parts] + [parts[-1][k][-1:]])
        elif k not in ("X", "U"):
            out[k] = torch.cat([p[k] for p in parts])
    out.update(viol=torch.stack(viol), lam=al.lam, rho=al.rho)
    return out
