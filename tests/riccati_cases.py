"""Inputs and the NumPy reference of the Riccati backward pass (include/dojo_hip.h "Batched iLQR"), shared by tests/test_riccati_references.py (no device)
and tests/test_riccati_gpu.py.  Nothing here touches the GPU.

The reference is written for a generic dtype: it runs in fp64 and in np.longdouble (hand-written Cholesky and substitutions; the products go through NumPy's
matmul, which handles both).  e_ref of a case is the distance between the two, per output array, relative to the array's largest entry; the gate of the GPU
test is 32 max(e_ref, 2^-52) max|ref| (+ 2^-23 max|ref| for fp32 handles).

Inputs: A = I + 0.1 N / sqrt(n), B = N / sqrt(n), lxx = M M^T + 0.1 I, luu = M M^T + I, lux = 0.1 N, lx, lu ~ N, seeded PER ENVIRONMENT: the inputs of
environment e do not depend on the batch it is put into (the bit-identity tests move environments between batches)."""
import numpy as np

U52, U23 = 2.0 ** -52, 2.0 ** -23
FACTOR = 32.0

# (mechanism, n = 2 nu, nu, act_off, na): the shapes of the GPU test
SHAPES = {
    "slider": ("slider", 2, 1, 0, 1),
    "cartpole1": ("cartpole", 4, 2, 0, 1),
    "cartpole2": ("cartpole", 4, 2, 0, 2),            # na = nu
    "ant": ("ant", 28, 14, 6, 8),
    "quadruped": ("quadruped", 36, 18, 6, 12),
    "atlas": ("atlas", 72, 36, 6, 30),
    "atlas5": ("atlas", 72, 36, 6, 5),                # n + na = 77: the 12-accumulator build
    "atlas36": ("atlas", 72, 36, 0, 36),              # na = nu: the largest plan (64 864 bytes of LDS)
}
# (shape, H, B): H over {1, 3, 20}, B over {1, 5, 65}; the large shapes take the small batches
CASES = [("slider", 1, 1), ("slider", 3, 5), ("slider", 20, 65),
         ("cartpole1", 20, 5), ("cartpole1", 3, 65), ("cartpole2", 1, 1), ("cartpole2", 3, 65),
         ("ant", 20, 5), ("ant", 3, 65), ("ant", 1, 1),
         ("quadruped", 20, 1), ("quadruped", 3, 5),
         ("atlas", 20, 1), ("atlas", 3, 5), ("atlas", 1, 65), ("atlas5", 3, 5), ("atlas36", 3, 1)]
OUTPUTS = ("K", "kff", "dV", "Vx", "Vxx")


def env_inputs(n, nu, act_off, m, H, e, seed=20):
    """the inputs of environment e: dict of fp64 arrays without the batch axis.  The columns of Bm outside act_off .. act_off + m - 1 are NaN: they are not read."""
    rng = np.random.default_rng([seed, n, nu, act_off, m, H, e])
    A = np.eye(n) + 0.1 * rng.standard_normal((H, n, n)) / np.sqrt(n)
    Bm = np.full((H, n, nu), np.nan)
    Bm[:, :, act_off:act_off + m] = rng.standard_normal((H, n, m)) / np.sqrt(n)
    M = rng.standard_normal((H + 1, n, n)); lxx = M @ M.transpose(0, 2, 1) + 0.1 * np.eye(n)
    M = rng.standard_normal((H, m, m)); luu = M @ M.transpose(0, 2, 1) + np.eye(m)
    return {"A": A, "Bm": Bm, "lx": rng.standard_normal((H + 1, n)), "lu": rng.standard_normal((H, m)), "lxx": lxx, "luu": luu,
            "lux": 0.1 * rng.standard_normal((H, m, n))}


def inputs(shape, H, B, f32=False, envs=None):
    """-> dict of fp64 arrays [H or H+1, B, ..] for the environments `envs` (default 0 .. B-1); f32: every value rounded to fp32 (what an fp32 handle is given)"""
    _, n, nu, act_off, m = SHAPES[shape]
    per = [env_inputs(n, nu, act_off, m, H, e) for e in (range(B) if envs is None else envs)]
    out = {k: np.ascontiguousarray(np.stack([p[k] for p in per], axis=1)) for k in per[0]}
    if f32:
        out = {k: v.astype(np.float32).astype(np.float64) for k, v in out.items()}
    return out


def cholesky(a):
    """lower Cholesky factor in a's dtype, column by column; None when a pivot is not > 0 or not finite"""
    m = a.shape[0]; L = np.zeros_like(a)
    for j in range(m):
        s = a[j:, j] - L[j:, :j] @ L[j, :j]
        d = s[0]
        if not (d > 0 and np.isfinite(d)):
            return None
        rd = np.sqrt(d)
        L[j, j] = rd; L[j + 1:, j] = s[1:] / rd
    return L


def cholesky_solve(L, rhs):
    """(L L^T)^-1 rhs, rhs [m, r], by forward and backward substitution in L's dtype"""
    m = L.shape[0]; x = np.array(rhs, dtype=L.dtype, copy=True)
    for i in range(m):
        x[i] = (x[i] - L[i, :i] @ x[:i]) / L[i, i]
    for i in range(m - 1, -1, -1):
        x[i] = (x[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def recursion(inp, act_off, m, mu=None, status=None, dtype=np.float64):
    """the recursion of include/dojo_hip.h, literally, per environment, in `dtype` -> dict K [H,B,m,n], kff [H,B,m], fail [B] int32, dV [B,2], Vx [B,n], Vxx [B,n,n]"""
    A, Bm = inp["A"], inp["Bm"]
    H, B, n = A.shape[:3]
    T = lambda x: np.asarray(x, dtype=dtype)
    out = {"K": np.zeros((H, B, m, n), dtype), "kff": np.zeros((H, B, m), dtype), "fail": np.zeros(B, np.int32), "dV": np.zeros((B, 2), dtype),
           "Vx": np.zeros((B, n), dtype), "Vxx": np.zeros((B, n, n), dtype)}
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
            L = cholesky(Qreg)
            if L is None:
                out["fail"][b] = k + 1
                out["K"][:k + 1, b] = 0; out["kff"][:k + 1, b] = 0
                Vx, Vxx, dV = np.zeros(n, dtype), np.zeros((n, n), dtype), np.zeros(2, dtype)
                break
            kff = -cholesky_solve(L, Qu[:, None])[:, 0]; K = -cholesky_solve(L, Qux)
            dV[0] += kff @ Qu; dV[1] += half * (kff @ Quu @ kff)
            Vx = Qx + K.T @ Quu @ kff + K.T @ Qu + Qux.T @ kff
            Vxx = Qxx + K.T @ Quu @ K + K.T @ Qux + Qux.T @ K
            Vxx = (Vxx + Vxx.T) * half
            out["K"][k, b], out["kff"][k, b] = K, kff
        out["dV"][b], out["Vx"][b], out["Vxx"][b] = dV, Vx, Vxx
    return out


_cache = {}


def reference(shape, H, B, f32=False):
    """-> (inputs, longdouble reference rounded to fp64, e_ref per output array): computed once per case and dtype, shared by the tests, never modified"""
    key = (shape, H, B, f32)
    if key not in _cache:
        _, n, nu, act_off, m = SHAPES[shape]
        inp = inputs(shape, H, B, f32)
        r64 = recursion(inp, act_off, m, dtype=np.float64)
        rld = recursion(inp, act_off, m, dtype=np.longdouble)
        assert not r64["fail"].any() and not rld["fail"].any()
        e = {k: float(np.abs(r64[k] - rld[k]).max() / np.abs(rld[k]).max()) for k in OUTPUTS}
        ref = {k: (rld[k].astype(np.float64) if k != "fail" else rld[k]) for k in rld}
        for v in list(inp.values()) + list(ref.values()):
            v.setflags(write=False)
        _cache[key] = (inp, ref, e)
    return _cache[key]


def bound(ref, e_ref, f32):
    """the gate of one output array: 32 max(e_ref, 2^-52) max|ref| (+ 2^-23 max|ref| for fp32 handles)"""
    top = float(np.abs(ref).max())
    return FACTOR * max(e_ref, U52) * top + (U23 * top if f32 else 0.0)
