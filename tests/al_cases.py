"""Inputs and the NumPy reference of the constrained Riccati backward pass (include/dojo_hip_constraints.h), shared by tests/test_riccati_al_references.py (no
device), tests/test_riccati_al_gpu.py and tests/test_ilqr_constrained_gpu.py.  Nothing here touches the GPU.

Inputs: those of riccati_cases.inputs (and, for the limited cases, box_cases.controls / limits) and, seeded per environment like them, nc constraint rows per
stage: G = [Cx Cu] = N / sqrt(n + m) (well scaled), y ~ N, and per row one of three states -- a quarter DEAD (w = y = 0: never loaded), an eighth w = 0 with
y != 0 (a multiplier without a penalty), the rest w = 10^U(-1, 3) <= 1e3.

The reference is the recursion of the header for a generic dtype, built from the pieces of box_cases and riccati_cases (the QP, the Cholesky, the margin); it runs
in fp64 and in np.longdouble and skips the rows the kernel does not load.  e_ref and the gate are riccati_cases' (bound)."""
import numpy as np

import box_cases as BC
import riccati_cases as RC

# rows per stage: ant 17 = a full block of 16 and a partial one, quadruped 16 = exactly one block, atlas 33 = three blocks
NC = {"slider": 1, "cartpole1": 4, "cartpole2": 4, "ant": 17, "quadruped": 16, "atlas5": 33, "atlas": 33}
# (shape, H, B): H over {1, 3}, B over {1, 5, 65}; atlas at B = 5 only
CASES = [("slider", 1, 1), ("slider", 3, 5), ("slider", 3, 65), ("cartpole1", 3, 5), ("cartpole1", 1, 65), ("cartpole2", 1, 1), ("cartpole2", 3, 65),
         ("ant", 1, 1), ("ant", 3, 5), ("ant", 3, 65), ("quadruped", 1, 1), ("quadruped", 3, 5), ("atlas5", 1, 5), ("atlas5", 3, 5), ("atlas", 1, 5), ("atlas", 3, 5)]
LIMITED_CASES = [("cartpole2", 3, 5), ("ant", 3, 5), ("atlas", 3, 5)]         # limits (box_cases' main family, c = 0.25) and constraints together
OUTPUTS = RC.OUTPUTS
W_MAX = 1.0e3


def env_constraints(n, m, nc, H, e, seed=22):
    """the constraint rows of environment e: dict Cx [H+1, nc, n], Cu [H, nc, m], w, y [H+1, nc] (fp64, without the batch axis)"""
    rng = np.random.default_rng([seed, n, m, nc, H, e])
    Cx = rng.standard_normal((H + 1, nc, n)) / np.sqrt(n + m); Cu = rng.standard_normal((H, nc, m)) / np.sqrt(n + m)
    w = 10.0 ** rng.uniform(-1.0, 3.0, (H + 1, nc)); y = rng.standard_normal((H + 1, nc))
    state = rng.uniform(0.0, 1.0, (H + 1, nc))
    w[state < 0.375] = 0.0; y[state < 0.25] = 0.0
    return {"Cx": Cx, "Cu": Cu, "w": w, "y": y}


def constraints(shape, H, B, f32=False, envs=None, nc=None):
    """-> dict Cx [H+1, B, nc, n], Cu [H, B, nc, m], w, y [H+1, B, nc]; f32: every value rounded to fp32"""
    _, n, nu, act_off, m = RC.SHAPES[shape]
    nc = NC[shape] if nc is None else nc
    per = [env_constraints(n, m, nc, H, e) for e in (range(B) if envs is None else envs)]
    out = {k: np.ascontiguousarray(np.stack([p[k] for p in per], axis=1)) for k in per[0]}
    if f32:
        out = {k: v.astype(np.float32).astype(np.float64) for k, v in out.items()}
    return out


def live(w, y):
    """the rows the kernel loads: every row but those with w = 0 and y = 0"""
    return ~((np.asarray(w) == 0) & (np.asarray(y) == 0))


def replicated(con, H, B):
    """a constraints dict whose Cx [nc, n], Cu [nc, m] are shared -> the same with them replicated over the stages and the batch"""
    out = dict(con)
    out["Cx"] = np.ascontiguousarray(np.broadcast_to(con["Cx"], (H + 1, B) + con["Cx"].shape))
    if con.get("Cu") is not None:
        out["Cu"] = np.ascontiguousarray(np.broadcast_to(con["Cu"], (H, B) + con["Cu"].shape))
    return out


def terms(con, k, b, n, m, dtype):
    """G' diag(w) G [N, N] and G' y [N] of stage k of environment b over the live rows (None, None: no live row); at k = H only the state part exists"""
    H = con["w"].shape[0] - 1
    w, y = con["w"][k, b], con["y"][k, b]
    lv = live(w, y)
    if not lv.any():
        return None, None
    T = lambda x: np.asarray(x, dtype=dtype)
    nc = len(w)
    Cu = con.get("Cu")
    G = np.zeros((nc, n + (m if k < H else 0)), dtype)
    G[:, :n] = np.where(lv[:, None], T(con["Cx"][k, b]), dtype(0))
    if k < H and Cu is not None:
        G[:, n:] = np.where(lv[:, None], T(Cu[k, b]), dtype(0))
    w_, y_ = np.where(lv, T(w), dtype(0)), np.where(lv, T(y), dtype(0))
    return G.T @ (w_[:, None] * G), G.T @ y_


def recursion(inp, con, act_off, m, U=None, lo=None, hi=None, mu=None, status=None, dtype=np.float64):
    """the recursion of include/dojo_hip_constraints.h, per environment, in `dtype`.  con: the dict of `constraints` (Cu may be None; None or nc = 0: no rows);
    U, lo, hi as in box_cases.recursion (all None: no limits) -> the dict of box_cases.recursion"""
    A, Bm = inp["A"], inp["Bm"]
    H, B, n = A.shape[:3]
    T = lambda x: np.asarray(x, dtype=dtype)
    out = {"K": np.zeros((H, B, m, n), dtype), "kff": np.zeros((H, B, m), dtype), "fail": np.zeros(B, np.int32), "dV": np.zeros((B, 2), dtype),
           "Vx": np.zeros((B, n), dtype), "Vxx": np.zeros((B, n, n), dtype), "active": np.zeros((H, B), np.int64), "iters": np.zeros((H, B), np.int32),
           "mask": np.zeros((H, B, m), bool), "margin": np.full((H, B), np.inf)}
    half = dtype(0.5)
    rows = con is not None and con["w"].shape[-1] > 0
    for b in range(B):
        Vx, Vxx = T(inp["lx"][H, b]), T(inp["lxx"][H, b])
        if rows:
            P, p = terms(con, H, b, n, m, dtype)
            if P is not None:
                Vxx = Vxx + P; Vx = Vx + p
        dV = np.zeros(2, dtype)
        for k in range(H - 1, -1, -1):
            if status is not None and status[k, b] != 0:
                Ak, Bk = np.zeros((n, n), dtype), np.zeros((n, m), dtype)
            else:
                Ak, Bk = T(A[k, b]), T(Bm[k, b][:, act_off:act_off + m])
            lux = T(inp["lux"][k, b]) if inp.get("lux") is not None else np.zeros((m, n), dtype)
            Qx = T(inp["lx"][k, b]) + Ak.T @ Vx; Qu = T(inp["lu"][k, b]) + Bk.T @ Vx
            Qxx = T(inp["lxx"][k, b]) + Ak.T @ Vxx @ Ak; Qux = lux + Bk.T @ Vxx @ Ak; Quu = T(inp["luu"][k, b]) + Bk.T @ Vxx @ Bk
            if rows:
                P, p = terms(con, k, b, n, m, dtype)
                if P is not None:
                    Qxx = Qxx + P[:n, :n]; Qux = Qux + P[n:, :n]; Quu = Quu + P[n:, n:]; Qx = Qx + p[:n]; Qu = Qu + p[n:]
            Qreg = Quu + (T(mu[b]) if mu is not None else dtype(0)) * np.eye(m, dtype=dtype)
            u = T(U[k, b, act_off:act_off + m]) if U is not None else np.zeros(m, dtype)
            lo_ = T(lo[b]) - u if lo is not None else np.full(m, -np.inf, dtype)
            hi_ = T(hi[b]) - u if hi is not None else np.full(m, np.inf, dtype)
            code, qp = 0, None
            if not (lo_ <= hi_).all():
                code = -(k + 1)
            else:
                L = RC.cholesky(Qreg)
                if L is None:
                    code = k + 1
                else:
                    qp = BC.box_qp(Qreg, Qu, L, lo_, hi_)
                    if qp is None:
                        code = -(k + 1)
            if code:
                out["fail"][b] = code
                out["K"][:k + 1, b] = 0; out["kff"][:k + 1, b] = 0; out["active"][:k + 1, b] = 0; out["iters"][:k + 1, b] = 0; out["mask"][:k + 1, b] = False
                Vx, Vxx, dV = np.zeros(n, dtype), np.zeros((n, n), dtype), np.zeros(2, dtype)
                break
            kff, cl, it, g = qp
            if cl.any():
                K = -RC.cholesky_solve(RC.cholesky(BC.masked(Qreg, cl)), np.where(cl[:, None], dtype(0), Qux))
                K[cl] = 0
            else:
                K = -RC.cholesky_solve(L, Qux)
            dV[0] += kff @ Qu; dV[1] += half * (kff @ Quu @ kff)
            Vx = Qx + K.T @ Quu @ kff + K.T @ Qu + Qux.T @ kff
            Vxx = Qxx + K.T @ Quu @ K + K.T @ Qux + Qux.T @ K
            Vxx = (Vxx + Vxx.T) * half
            out["K"][k, b], out["kff"][k, b] = K, kff
            out["mask"][k, b] = cl; out["active"][k, b] = np.array(sum(1 << i for i in range(m) if cl[i]), np.uint64).astype(np.int64)
            out["iters"][k, b] = it
            out["margin"][k, b] = BC.margin(np.asarray(kff, np.float64), cl, np.asarray(g, np.float64), np.asarray(Qu, np.float64), np.asarray(lo_, np.float64), np.asarray(hi_, np.float64))
        out["dV"][b], out["Vx"][b], out["Vxx"][b] = dV, Vx, Vxx
    return out


def folded(inp, con, m):
    """the same problem for box_cases.recursion: the constraint terms formed into lx, lu, lxx, luu, lux in fp64 (what the kernel never writes to memory)"""
    H, B, n = inp["A"].shape[:3]
    out = {k: np.array(v, copy=True) for k, v in inp.items()}
    for b in range(B):
        for k in range(H + 1):
            P, p = terms(con, k, b, n, m, np.float64)
            if P is None:
                continue
            out["lxx"][k, b] += P[:n, :n]; out["lx"][k, b] += p[:n]
            if k < H:
                out["lux"][k, b] += P[n:, :n]; out["luu"][k, b] += P[n:, n:]; out["lu"][k, b] += p[n:]
    return out


_cache = {}


def reference(shape, H, B, f32=False, limited=False):
    """-> (inputs, constraints, U, lo, hi (None without limits), longdouble reference rounded to fp64, e_ref per output array, the fp64 run): computed once per
    case and dtype, shared by the tests, never modified"""
    key = (shape, H, B, f32, limited)
    if key not in _cache:
        _, n, nu, act_off, m = RC.SHAPES[shape]
        inp = RC.inputs(shape, H, B, f32); con = constraints(shape, H, B, f32)
        U = lo = hi = None
        if limited:
            U = BC.controls(shape, H, B, BC.C_MAIN, f32); lo, hi = BC.limits(shape, B, BC.C_MAIN)
        r64 = recursion(inp, con, act_off, m, U, lo, hi, dtype=np.float64)
        rld = recursion(inp, con, act_off, m, U, lo, hi, dtype=np.longdouble)
        e = {k: float(np.abs(r64[k] - rld[k]).max() / np.abs(rld[k]).max()) for k in OUTPUTS}
        ref = {k: (v.astype(np.float64) if k in OUTPUTS else v) for k, v in rld.items()}
        for v in list(inp.values()) + list(con.values()) + list(ref.values()) + list(r64.values()) + [x for x in (U, lo, hi) if x is not None]:
            v.setflags(write=False)
        _cache[key] = (inp, con, U, lo, hi, ref, e, r64)
    return _cache[key]


# ---------------------------------------------------------------- the AL loop on linear-quadratic problems ----------------------------------------------------------------
def lq_cost(X, U, Q, R, Qf, xg):
    d = X - xg
    return 0.5 * np.einsum("ki,ij,kj->", d[:-1], Q, d[:-1]) + 0.5 * np.einsum("ki,ij,kj->", U, R, U) + 0.5 * d[-1] @ Qf @ d[-1]


def lq_weights(c, lam, rho, ineq, present):
    """the rule of ilqr.solve_constrained: a = present & (~ineq | c >= 0 | lam > 0), w = rho a, y = lam + w c"""
    a = present & (~ineq[None, :] | (c >= 0) | (lam > 0))
    w = rho * a
    return w, lam + w * c


def lq_violation(c, ineq, present):
    v = np.where(ineq[None, :], np.maximum(c, 0.0), np.abs(c)) * present
    return float(v.max()) if v.size else 0.0


def al_loop_lq(A, Bm, X, U, Q, R, Qf, xg, Cx, d, ineq, present, outer, iters=1, rho0=1.0, rho_scale=10.0, rho_max=1e8, dtype=np.float64, A_roll=None, B_roll=None):
    """The augmented-Lagrangian loop of ilqr.solve_constrained on ONE environment whose dynamics are affine: A [H, n, n], Bm [H, n, m] are exact along any
    trajectory, (X, U) is the start trajectory, the constraints are c_k = Cx x_k - d ([nc, n], [nc]; present [H+1, nc], ineq [nc]).  Every inner iteration is the
    recursion above with the full step a = 1 (exact for an affine problem).  A_roll, B_roll: the maps the forward pass follows where they are not the A, Bm of the
    backward pass (the device linearizes with the reference's regularised solve, so its Jacobians are those of the steps only to 1e-10; its rollouts follow the
    steps).  -> dict viol [outer + 1], J [outer iters + 1], lam, rho, X, U"""
    H, n, m = Bm.shape
    nc = Cx.shape[0]
    X, U = np.array(X, dtype), np.array(U, dtype)
    A_roll, B_roll = A if A_roll is None else A_roll, Bm if B_roll is None else B_roll
    lam = np.zeros((H + 1, nc), dtype); rho = dtype(rho0)
    cons = lambda X: (X @ Cx.T - d) * present
    viol, J = [lq_violation(cons(X), ineq, present)], [float(lq_cost(X, U, Q, R, Qf, xg))]
    for _ in range(outer):
        for _ in range(iters):
            c = cons(X)
            w, y = lq_weights(c, lam, rho, ineq, present)
            dx = X - xg
            inp = {"A": A[:, None], "Bm": Bm[:, None], "lx": np.concatenate([dx[:-1] @ Q.T, (dx[-1] @ Qf.T)[None]])[:, None], "lu": (U @ R.T)[:, None],
                   "lxx": np.concatenate([np.broadcast_to(Q, (H, n, n)), Qf[None]])[:, None], "luu": np.broadcast_to(R, (H, 1, m, m)), "lux": None}
            con = {"Cx": np.broadcast_to(Cx, (H + 1, 1, nc, n)), "Cu": None, "w": w[:, None], "y": y[:, None]}
            r = recursion(inp, con, 0, m, dtype=dtype)
            assert r["fail"][0] == 0
            Xn, Un = X.copy(), U.copy()
            for k in range(H):
                du = r["kff"][k, 0] + r["K"][k, 0] @ (Xn[k] - X[k])
                Un[k] = U[k] + du
                Xn[k + 1] = X[k + 1] + A_roll[k] @ (Xn[k] - X[k]) + B_roll[k] @ du
            X, U = Xn, Un
            J.append(float(lq_cost(X, U, Q, R, Qf, xg)))
        c = cons(X)
        viol.append(lq_violation(c, ineq, present))
        lam = np.where(present, np.where(ineq[None, :], np.maximum(0.0, lam + rho * c), lam + rho * c), lam)
        rho = min(rho_scale * rho, rho_max)
    return {"viol": np.array(viol), "J": np.array(J), "lam": lam, "rho": rho, "X": X, "U": U}


def kkt_lq(A, Bm, x0, aff, Q, R, Qf, xg, Cx, d):
    """the dense KKT solution of  min J  s.t.  x_{k+1} = A_k x_k + B_k u_k + aff_k,  Cx x_H = d  (a terminal equality) -> X [H+1, n], U [H, m]"""
    H, n, m = Bm.shape
    # x_H and every x_k as affine functions of the stacked controls: x_k = Sx[k] + Su[k] u
    Sx, Su = [np.array(x0, float)], [np.zeros((n, H * m))]
    for k in range(H):
        S = A[k] @ Su[k]; S[:, k * m:(k + 1) * m] += Bm[k]
        Sx.append(A[k] @ Sx[k] + aff[k]); Su.append(S)
    Hq, g = np.kron(np.eye(H), R), np.zeros(H * m)
    for k in range(H + 1):
        W = Qf if k == H else Q
        Hq = Hq + Su[k].T @ W @ Su[k]; g = g + Su[k].T @ W @ (Sx[k] - xg)
    E, f = Cx @ Su[H], d - Cx @ Sx[H]
    nc = E.shape[0]
    sol = np.linalg.solve(np.block([[Hq, E.T], [E, np.zeros((nc, nc))]]), np.concatenate([-g, f]))
    u = sol[:H * m]
    return np.stack([Sx[k] + Su[k] @ u for k in range(H + 1)]), u.reshape(H, m)
