"""The seeded synthetic cases of the line-search selection (include/dojo_hip_linesearch.h, dojo_linesearch_select_dev) and its NumPy reference, shared by
tests/test_linesearch_references.py (no device) and tests/test_linesearch_gpu.py.  Nothing here touches the GPU and nothing is stepped: the trials are made up.

The shapes are those of minimal_cases.SHAPES.  Everything is seeded PER PROBLEM: the inputs of problem p do not depend on P (the bit-identity tests compare
P = 5 with the first 5 problems of P = 65).  The cost matrices and the goal are shared by the problems and seeded by the shape.

Trial tr of problem p, around the current trajectory (Xcur, Ucur) with cost J0:
    X = goal + g (Xcur - goal) (1 + 0.01 N(0, 1)),  U = g Ucur,   g = 1.3 for tr < target, 0.8 from the target on -- J is about 1.69 J0 / 0.64 J0 --,
    target = p mod (T + 1) (T: no trial is acceptable); a trial behind target + 1 goes back to 1.3 with probability 0.3: first != last != best
    dV = (-0.1 J0, 0.02 J0),  alpha = 2^-tr,  c1 = 1e-4: the threshold is J0 (1 - O(1e-5)), about 0.3 J0 away from every trial
Planted on top: p mod 7 = 1: a failed step in the target trial;  p mod 11 = 7: ok = 0;  p mod 13 = 4: one NaN state in the target trial (its cost is NaN)."""
import numpy as np

from minimal_cases import SHAPES
from riccati_cases import FACTOR, U52

C1 = 1e-4
# (shape, H, T, P): H over 1 / 3, T over 1 / 3 / 8 / 9 (one trial; fewer trials than the wavefronts of a workgroup; two full rounds of them; a round with one left
# over), P over 1 / 5 / 65; atlas at T = 3, P = 5, H = 2 only
CASES = [(s, H, T, P) for s in ("slider", "cartpole1", "cartpole2", "ant")
         for H, T, P in ((1, 1, 1), (3, 3, 5), (3, 3, 65), (1, 8, 5), (3, 8, 65), (3, 9, 5), (1, 9, 65), (3, 1, 65))] + [("atlas", 2, 3, 5)]


def shared(shape):
    """Q, R, Qf, goal of a shape: M M' / size + I, goal ~ N(0, 1)"""
    _, n, nu, act_off, m = SHAPES[shape]
    rng = np.random.default_rng([57, n, nu, act_off, m])
    spd = lambda k: (lambda M: M @ M.T / k + np.eye(k))(rng.standard_normal((k, k)))
    return {"Q": spd(n), "R": spd(m), "Qf": spd(n), "goal": rng.standard_normal(n)}


def cost(X, U_act, c, dtype=np.float64):
    """ilqr.QuadraticCost.value in `dtype`: X [H+1, .., n], U_act [H, .., na] -> J [..]"""
    T = lambda a: np.asarray(a, dtype=dtype)
    d = T(X) - T(c["goal"])
    half = dtype(0.5)
    J = half * ((d[:-1] @ T(c["Q"]).T) * d[:-1]).sum((0, -1)) + half * ((T(U_act) @ T(c["R"]).T) * T(U_act)).sum((0, -1))
    return J + half * ((d[-1] @ T(c["Qf"]).T) * d[-1]).sum(-1)


def problem(shape, H, T, p):
    """the inputs of problem p without the batch axis: Xcur [H+1,n], Ucur [H,nu], X [T,H+1,n], U [T,H,nu], status [T,H], alpha [T], dV [2], ok, and the plants"""
    _, n, nu, act_off, m = SHAPES[shape]
    c = shared(shape)
    rng = np.random.default_rng([58, n, nu, act_off, m, H, T, p])
    Xcur = c["goal"] + rng.standard_normal((H + 1, n)); Ucur = rng.standard_normal((H, nu))
    J0 = float(cost(Xcur, Ucur[:, act_off:act_off + m], c))
    target = p % (T + 1)
    g = np.where(np.arange(T) < target, 1.3, 0.8)
    back = rng.random(T) < 0.3
    g[(np.arange(T) > target + 1) & back] = 1.3
    noise = 1.0 + 0.01 * rng.standard_normal((T, H + 1, n))
    X = c["goal"] + g[:, None, None] * (Xcur - c["goal"])[None] * noise
    U = g[:, None, None] * Ucur[None]
    status = np.zeros((T, H), np.int32)
    plants = {"status": p % 7 == 1 and target < T, "ok": p % 11 == 7, "nan": p % 13 == 4 and target < T}
    if plants["status"]:
        status[target, int(rng.integers(H))] = 1 + int(rng.integers(2))
    if plants["nan"]:
        X[target, int(rng.integers(H + 1)), int(rng.integers(n))] = np.nan
    return {"Xcur": Xcur, "Ucur": Ucur, "X": X, "U": U, "status": status, "alpha": 2.0 ** -np.arange(T), "dV": np.array([-0.1 * J0, 0.02 * J0]),
            "ok": np.int32(0 if plants["ok"] else 1)}, plants


_inputs = {}


def inputs(shape, H, T, P, f32=False):
    """-> (dict of arrays in the ABI's layouts -- X [H+1,T P,n], U [H,T P,nu], status [H,T P], alpha [T,P], dV [P,2], ok [P], Xcur [H+1,P,n], Ucur [H,P,nu], Q, R, Qf,
    goal; floats as fp64, rounded to fp32 values with f32: what an fp32 handle is given --, plants: three [P] bool arrays).  Cached and read-only."""
    key = (shape, H, T, P, f32)
    if key not in _inputs:
        _, n, nu, act_off, m = SHAPES[shape]
        per = [problem(shape, H, T, p) for p in range(P)]
        st = lambda k, axis: np.stack([q[0][k] for q in per], axis=axis)
        inp = {"X": st("X", 2).transpose(1, 0, 2, 3).reshape(H + 1, T * P, n), "U": st("U", 2).transpose(1, 0, 2, 3).reshape(H, T * P, nu),
               "status": st("status", 2).transpose(1, 0, 2).reshape(H, T * P), "alpha": st("alpha", 1), "dV": st("dV", 0), "ok": st("ok", 0).astype(np.int32),
               "Xcur": st("Xcur", 1), "Ucur": st("Ucur", 1), **shared(shape)}
        inp = {k: np.ascontiguousarray(v) for k, v in inp.items()}
        if f32:
            inp = {k: (v if v.dtype == np.int32 else v.astype(np.float32).astype(np.float64)) for k, v in inp.items()}
        plants = {k: np.array([q[1][k] for q in per]) for k in ("status", "ok", "nan")}
        for v in list(inp.values()) + list(plants.values()):
            v.setflags(write=False)
        _inputs[key] = (inp, plants)
    return _inputs[key]


def select(inp, shape, T, dtype=np.float64, J_trial=None, J0=None, use_status=True, use_ok=True):
    """the selection of include/dojo_hip_linesearch.h in `dtype` -> dict J_trial [T,P], J_cur [P], thr [T,P], choice [P] int32, alpha [P], J_acc [P], X [H+1,P,n],
    U [H,P,nu].  J_trial / J0 given: the mode without a cost."""
    _, n, nu, act_off, m = SHAPES[shape]
    H, B = inp["U"].shape[:2]
    P = B // T
    act = slice(act_off, act_off + m)
    if J_trial is None:
        with np.errstate(invalid="ignore"):
            J_trial = cost(inp["X"], inp["U"][:, :, act], inp, dtype).reshape(T, P)
    if J0 is None:
        J0 = cost(inp["Xcur"], inp["Ucur"][:, :, act], inp, dtype)
    J_trial, J0 = np.asarray(J_trial, dtype=dtype), np.asarray(J0, dtype=dtype)
    a, dV = np.asarray(inp["alpha"], dtype=dtype), np.asarray(inp["dV"], dtype=dtype)
    thr = J0[None] + dtype(C1) * (a * dV[None, :, 0] + a * a * dV[None, :, 1])
    solved = (inp["status"].reshape(H, T, P) == 0).all(0) if use_status else np.ones((T, P), bool)
    with np.errstate(invalid="ignore"):
        acceptable = solved & (J_trial <= thr) & ((inp["ok"] != 0)[None] if use_ok else True)
    choice = np.where(acceptable.any(0), acceptable.argmax(0), -1).astype(np.int32)
    pick, cols = np.maximum(choice, 0), np.arange(P)
    yes = choice >= 0
    Xt, Ut = inp["X"].reshape(H + 1, T, P, n), inp["U"].reshape(H, T, P, nu)
    return {"J_trial": J_trial, "J_cur": J0, "thr": thr, "choice": choice, "alpha": np.where(yes, a[pick, cols], 0), "J_acc": np.where(yes, J_trial[pick, cols], J0),
            "X": np.where(yes[None, :, None], Xt[:, pick, cols], inp["Xcur"]), "U": np.where(yes[None, :, None], Ut[:, pick, cols], inp["Ucur"])}


COSTS = ("J_trial", "J_cur", "J_acc")
_refs = {}


def reference(shape, H, T, P, f32=False):
    """-> (inputs, plants, the longdouble reference with its costs rounded to fp64, e_ref per cost array: the distance between the fp64 and the longdouble
    evaluation relative to the array's largest finite entry).  Computed once per case and dtype, shared by the tests, never modified."""
    key = (shape, H, T, P, f32)
    if key not in _refs:
        inp, plants = inputs(shape, H, T, P, f32)
        r64, rld = select(inp, shape, T, np.float64), select(inp, shape, T, np.longdouble)
        assert (r64["choice"] == rld["choice"]).all()
        e = {k: float(np.nanmax(np.abs(r64[k] - rld[k])) / np.nanmax(np.abs(rld[k]))) for k in COSTS}
        ref = {k: (np.asarray(v, dtype=np.float64) if k in COSTS + ("thr", "alpha") else v) for k, v in rld.items()}
        for v in ref.values():
            v.setflags(write=False)
        _refs[key] = (inp, plants, ref, e)
    return _refs[key]


def bound(ref, e_ref):
    """the gate of one cost array: 32 max(e_ref, 2^-52) max|ref| -- riccati_cases.bound without the fp32 term, because these arrays are double"""
    return FACTOR * max(e_ref, U52) * float(np.nanmax(np.abs(ref)))
