"""Inputs and the NumPy reference of the control-limited Riccati backward pass (include/dojo_hip_limits.h), shared by tests/test_riccati_box_references.py (no
device) and tests/test_riccati_box_gpu.py.  Nothing here touches the GPU.

Inputs: those of riccati_cases.inputs, the controls U[k][e] = clip(0.5 N(0, 1), -c, c) seeded per environment and step, and the limits lo = -c, hi = +c;
c = 0.25 is the main family (a third to nine tenths of the inputs end clamped), c = 1.0 a second one (few do).

The reference is the recursion of the header for a generic dtype, with riccati_cases.cholesky and riccati_cases.cholesky_solve: it runs in fp64 and in
np.longdouble.  e_ref and the gate are those of riccati_cases (bound).  Per step it also returns the strict-complementarity margin of the solution: the smaller
of min |g_i| / max(1, max|Qu|) over the clamped i and the smallest distance of a free x_i to its bounds -- the clamped set, and with it K, is only determined
where that is not tiny."""
import itertools

import numpy as np

import riccati_cases as RC

C_MAIN, C_WIDE = 0.25, 1.0
CS = (C_MAIN, C_WIDE)
# (shape, H, B): the smallest that reach every accumulator build, m = 1, m = nu, more than one workgroup's worth of environments, and a horizon long
# enough for clamped steps to feed later ones
CASES = [("slider", 3, 5), ("cartpole1", 3, 5), ("cartpole2", 3, 65), ("ant", 3, 5), ("ant", 20, 5), ("quadruped", 3, 5), ("atlas", 3, 5), ("atlas5", 3, 5)]
GPU_CASES = CASES + [("atlas36", 3, 1)]           # ... and the largest plan that fits: na = nu = 36
OUTPUTS = RC.OUTPUTS
MAX_ITERS, MAX_TRIALS = 64, 40


def env_controls(nu, H, e, c, seed=21):
    """U [H, nu] of environment e: every step has its own stream, so an environment's controls depend neither on the batch nor on the horizon above the step"""
    return np.stack([np.clip(0.5 * np.random.default_rng([seed, nu, e, k]).standard_normal(nu), -c, c) for k in range(H)])


def controls(shape, H, B, c, f32=False, envs=None):
    """-> U [H, B, nu] fp64 (f32: rounded to fp32 values)"""
    nu = RC.SHAPES[shape][2]
    U = np.ascontiguousarray(np.stack([env_controls(nu, H, e, c) for e in (range(B) if envs is None else envs)], axis=1))
    return U.astype(np.float32).astype(np.float64) if f32 else U


def limits(shape, B, c):
    """-> lo, hi [B, m] (c is a value of both ABI types)"""
    m = RC.SHAPES[shape][4]
    return np.full((B, m), -float(c)), np.full((B, m), float(c))


def masked(Qreg, cl):
    """Qreg with the rows and columns of the clamped set replaced by the identity's"""
    M = Qreg.copy()
    M[cl, :] = 0; M[:, cl] = 0
    M[cl, cl] = 1
    return M


def box_qp(Qreg, Qu, L, lo, hi):
    """argmin 1/2 x' Qreg x + Qu' x over lo <= x <= hi by the projected Newton of the header, in Qreg's dtype; L = cholesky(Qreg).
    -> (x, clamped mask, iterations, g) or None: more than 64 iterations, no accepted step length, or a bad pivot of a masked factor"""
    dtype = Qreg.dtype.type
    m = len(Qu)
    x0 = -RC.cholesky_solve(L, Qu[:, None])[:, 0]
    x = np.minimum(np.maximum(x0, lo), hi)
    if (x == x0).all():
        return x0, np.zeros(m, bool), 0, Qu + Qreg @ x0
    tol = dtype(64) * np.finfo(dtype).eps
    qumax, qmax = np.abs(Qu).max(), np.abs(Qreg).max()
    prev, prev_full, it = None, False, 0
    while True:
        g = Qu + Qreg @ x
        cl = ((x <= lo) & (g > 0)) | ((x >= hi) & (g < 0))
        free = ~cl
        if not free.any() or (prev is not None and (cl == prev).all() and prev_full) or np.abs(g[free]).max() <= tol * max(qumax, qmax * np.abs(x).max()):
            return x, cl, it, g
        if it == MAX_ITERS:
            return None
        it += 1
        Lm = RC.cholesky(masked(Qreg, cl))
        if Lm is None:
            return None
        d = -RC.cholesky_solve(Lm, np.where(cl, dtype(0), g)[:, None])[:, 0]
        s, accepted = dtype(1), False
        for _ in range(MAX_TRIALS):
            xu = x + s * d
            xt = np.minimum(np.maximum(xu, lo), hi)
            dx = xt - x
            gd = g @ dx
            if gd + dtype(0.5) * (dx @ Qreg @ dx) <= dtype(0.1) * gd:
                accepted = True
                break
            s = s * dtype(0.5)
        if not accepted:
            return None
        prev, prev_full, x = cl, bool(s == 1 and (xt == xu).all()), xt


def margin(x, cl, g, Qu, lo, hi):
    """strict complementarity of a solution: min(min over clamped |g_i| / max(1, max|Qu|), min over free of the distance to the bounds); inf where a set is empty"""
    a = float((np.abs(g[cl]) / max(1.0, float(np.abs(Qu).max()))).min()) if cl.any() else np.inf
    f = ~cl
    b = float(np.minimum(x[f] - lo[f], hi[f] - x[f]).min()) if f.any() else np.inf
    return min(a, b)


def recursion(inp, U, lo, hi, act_off, m, mu=None, status=None, dtype=np.float64):
    """the recursion of include/dojo_hip_limits.h, literally, per environment, in `dtype`.  lo, hi [B, m] (None: no limit on that side), U [H, B, nu].
    -> dict K, kff, fail, dV, Vx, Vxx as riccati_cases.recursion, active [H,B] int64, iters [H,B] int32, mask [H,B,m] bool, margin [H,B]"""
    A, Bm = inp["A"], inp["Bm"]
    H, B, n = A.shape[:3]
    T = lambda x: np.asarray(x, dtype=dtype)
    out = {"K": np.zeros((H, B, m, n), dtype), "kff": np.zeros((H, B, m), dtype), "fail": np.zeros(B, np.int32), "dV": np.zeros((B, 2), dtype),
           "Vx": np.zeros((B, n), dtype), "Vxx": np.zeros((B, n, n), dtype), "active": np.zeros((H, B), np.int64), "iters": np.zeros((H, B), np.int32),
           "mask": np.zeros((H, B, m), bool), "margin": np.full((H, B), np.inf)}
    half = dtype(0.5)
    for b in range(B):
        Vx, Vxx = T(inp["lx"][H, b]), T(inp["lxx"][H, b])
        dV = np.zeros(2, dtype)
        for k in range(H - 1, -1, -1):
            if status is not None and status[k, b] != 0:
                Ak, Bk = np.zeros((n, n), dtype), np.zeros((n, m), dtype)
            else:
                Ak, Bk = T(A[k, b]), T(Bm[k, b][:, act_off:act_off + m])
            lux = T(inp["lux"][k, b]) if inp.get("lux") is not None else np.zeros((m, n), dtype)
            Qx = T(inp["lx"][k, b]) + Ak.T @ Vx; Qu = T(inp["lu"][k, b]) + Bk.T @ Vx
            Qxx = T(inp["lxx"][k, b]) + Ak.T @ Vxx @ Ak; Qux = lux + Bk.T @ Vxx @ Ak; Quu = T(inp["luu"][k, b]) + Bk.T @ Vxx @ Bk
            Qreg = Quu + (T(mu[b]) if mu is not None else dtype(0)) * np.eye(m, dtype=dtype)
            u = T(U[k, b, act_off:act_off + m])
            lo_ = T(lo[b]) - u if lo is not None else np.full(m, -np.inf, dtype)
            hi_ = T(hi[b]) - u if hi is not None else np.full(m, np.inf, dtype)
            code = 0
            if not (lo_ <= hi_).all():
                code = -(k + 1)
            else:
                L = RC.cholesky(Qreg)
                if L is None:
                    code = k + 1
                else:
                    qp = box_qp(Qreg, Qu, L, lo_, hi_)
                    if qp is None:
                        code = -(k + 1)
            if code:
                out["fail"][b] = code
                out["K"][:k + 1, b] = 0; out["kff"][:k + 1, b] = 0; out["active"][:k + 1, b] = 0; out["iters"][:k + 1, b] = 0; out["mask"][:k + 1, b] = False
                Vx, Vxx, dV = np.zeros(n, dtype), np.zeros((n, n), dtype), np.zeros(2, dtype)
                break
            kff, cl, it, g = qp
            if cl.any():
                K = -RC.cholesky_solve(RC.cholesky(masked(Qreg, cl)), np.where(cl[:, None], dtype(0), Qux))
                K[cl] = 0
            else:
                K = -RC.cholesky_solve(L, Qux)
            dV[0] += kff @ Qu; dV[1] += half * (kff @ Quu @ kff)
            Vx = Qx + K.T @ Quu @ kff + K.T @ Qu + Qux.T @ kff
            Vxx = Qxx + K.T @ Quu @ K + K.T @ Qux + Qux.T @ K
            Vxx = (Vxx + Vxx.T) * half
            out["K"][k, b], out["kff"][k, b] = K, kff
            out["mask"][k, b] = cl; out["active"][k, b] = np.array(sum(1 << i for i in range(m) if cl[i]), np.uint64).astype(np.int64)      # (bit 63 of m = 64 wraps into the sign)
            out["iters"][k, b] = it
            out["margin"][k, b] = margin(np.asarray(kff, np.float64), cl, np.asarray(g, np.float64), np.asarray(Qu, np.float64), np.asarray(lo_, np.float64), np.asarray(hi_, np.float64))
        out["dV"][b], out["Vx"][b], out["Vxx"][b] = dV, Vx, Vxx
    return out


def brute_force(Qreg, Qu, lo, hi):
    """the same QP by enumeration (m <= 8): every one of the 3^m patterns free / at lo / at hi, its face solved with numpy.linalg.solve; the pattern that is
    feasible with multipliers of the right sign -> (x, clamped mask)"""
    m = len(Qu)
    for pat in itertools.product((0, 1, 2), repeat=m):
        pat = np.array(pat)
        if ((pat == 1) & ~np.isfinite(lo)).any() or ((pat == 2) & ~np.isfinite(hi)).any():
            continue
        f = pat == 0
        x = np.where(pat == 1, lo, np.where(pat == 2, hi, 0.0))
        if f.any():
            x[f] = np.linalg.solve(Qreg[np.ix_(f, f)], -(Qu[f] + Qreg[np.ix_(f, ~f)] @ x[~f]))
        g = Qu + Qreg @ x
        if (x[f] >= lo[f]).all() and (x[f] <= hi[f]).all() and (g[pat == 1] >= 0).all() and (g[pat == 2] <= 0).all():
            return x, ~f
    return None


def step_model(inp, ref, act_off, m, k, b):
    """Qreg (mu = 0) and Qu of step k of environment b as the recursion forms them, in fp64, from the reference's own value function above the step: only defined
    for k = H - 1 (the value function is the terminal cost) and, through a one-step recursion from there, k = H - 2"""
    H = inp["A"].shape[0]
    Vx, Vxx = inp["lx"][H, b], inp["lxx"][H, b]
    for kk in range(H - 1, k - 1, -1):
        Ak, Bk = inp["A"][kk, b], inp["Bm"][kk, b][:, act_off:act_off + m]
        Qx = inp["lx"][kk, b] + Ak.T @ Vx; Qu = inp["lu"][kk, b] + Bk.T @ Vx
        Qxx = inp["lxx"][kk, b] + Ak.T @ Vxx @ Ak; Qux = inp["lux"][kk, b] + Bk.T @ Vxx @ Ak; Quu = inp["luu"][kk, b] + Bk.T @ Vxx @ Bk
        if kk == k:
            return Quu, Qu
        K, kff = ref["K"][kk, b], ref["kff"][kk, b]
        Vx = Qx + K.T @ Quu @ kff + K.T @ Qu + Qux.T @ kff
        Vxx = Qxx + K.T @ Quu @ K + K.T @ Qux + Qux.T @ K
        Vxx = (Vxx + Vxx.T) * 0.5


_cache = {}


def reference(shape, H, B, c, f32=False):
    """-> (inputs, U, lo, hi, longdouble reference rounded to fp64 (mask, active, iters, margin, fail as they are), e_ref per output array, the fp64 run):
    computed once per case, c and dtype, shared by the tests, never modified"""
    key = (shape, H, B, c, f32)
    if key not in _cache:
        _, n, nu, act_off, m = RC.SHAPES[shape]
        inp = RC.inputs(shape, H, B, f32)
        U = controls(shape, H, B, c, f32); lo, hi = limits(shape, B, c)
        r64 = recursion(inp, U, lo, hi, act_off, m, dtype=np.float64)
        rld = recursion(inp, U, lo, hi, act_off, m, dtype=np.longdouble)
        e = {k: float(np.abs(r64[k] - rld[k]).max() / np.abs(rld[k]).max()) for k in OUTPUTS}
        ref = {k: (v.astype(np.float64) if k in OUTPUTS else v) for k, v in rld.items()}
        for v in [U, lo, hi] + list(ref.values()) + list(r64.values()):
            v.setflags(write=False)
        _cache[key] = (inp, U, lo, hi, ref, e, r64)
    return _cache[key]
