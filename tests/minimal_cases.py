"""The seeded cases of the rollout in minimal coordinates (include/dojo_hip_trajopt.h) and its control law in NumPy, shared by
tests/test_rollout_minimal_references.py (no device) and tests/test_rollout_minimal_gpu.py.  Nothing here touches the GPU.

The law is written for a generic dtype (float64, np.longdouble) and is given X[k]: the tests recompute U_out[k] from the X[k] a rollout returned.
Inputs are seeded PER ENVIRONMENT: those of environment e do not depend on the batch it is put into (the determinism tests compare the leading environments
of B = 1 / 5 / 65), and a shorter horizon is a prefix of a longer one.

    K ~ 0.1 N(0, 1), kff ~ 0.1 N(0, 1), Ubar = the synthetic controls of the environment + 0.1 N(0, 1) per step, x0 = the synthetic state in minimal coordinates,
    alpha = 1, 0, then (e + 1) / (e + 3): distinct per environment, with 0 and 1 among them.
    Xbar: the open-loop trajectory of Ubar from the perturbed start x0 + p N(0, 1) (p = 1 for the slider and the cartpole, where every state is a valid one and
    K dx is then of the size of the controls; 0.02 for the mechanisms with contacts), so that x - xbar != 0 -- made by the caller with the stepper it has
    (`with_reference`: the device's open-loop rollout in the GPU test, the oracle in the reference test)."""
import numpy as np

import dojo_amd as d
from dojo_amd import coords

HMAX = 3
PERTURB = {"slider": 1.0, "cartpole": 1.0, "ant": 0.02, "atlas": 0.02}
U53 = 2.0 ** -53

# (mechanism, n = 2 nu, nu, act_off, na)
SHAPES = {
    "slider": ("slider", 2, 1, 0, 1),
    "cartpole1": ("cartpole", 4, 2, 0, 1),
    "cartpole2": ("cartpole", 4, 2, 0, 2),            # na = nu
    "ant": ("ant", 28, 14, 6, 8),                     # branches, contacts in force
    "atlas": ("atlas", 72, 36, 6, 30),                # rows longer than the 64 lanes
}
# (shape, H, B): H over 1 / 3, B over 1 / 5 / 65; atlas at B = 5, H = 2 only
CASES = [(s, H, B) for s in ("slider", "cartpole1", "cartpole2", "ant") for H, B in ((1, 1), (3, 5), (3, 65), (1, 65))] + [("atlas", 2, 5)]

_specs = {}


def spec_of(shape):
    name = SHAPES[shape][0]
    if name not in _specs:
        _specs[name] = {"ant": lambda: d.baseline_config(3), "atlas": lambda: d.baseline_config(5), "cartpole": d.get_cartpole}.get(name, lambda: d.get_mechanism(name))()
    return _specs[name]


_cache = {}


def _start(shape, B):
    """x0 [B,n], u [B,nu] of the synthetic inputs (row b depends on b alone)"""
    key = (SHAPES[shape][0], B)
    if key not in _cache:
        spec = spec_of(shape)
        Z, U = d.synthetic_inputs(spec, B)
        _cache[key] = (np.stack([coords.maximal_to_minimal(spec, z) for z in Z]), U)
    return _cache[key]


def inputs(shape, H, B, f32=False, envs=None):
    """-> dict of fp64 arrays: x0 [B,n], xbar0 [B,n] (the perturbed start of the reference trajectory), Ubar [H,B,nu], K [H,B,na,n], kff [H,B,na], alpha [B], for the
    environments `envs` (default 0 .. B-1); f32: every value rounded to fp32 (what an fp32 handle is given)"""
    name, n, nu, act_off, m = SHAPES[shape]
    envs = list(range(B) if envs is None else envs)
    x0s, us = _start(shape, max(envs) + 1)
    out = {k: [] for k in ("x0", "xbar0", "Ubar", "K", "kff", "alpha")}
    for e in envs:
        rng = np.random.default_rng([41, n, nu, act_off, m, e])
        out["x0"].append(x0s[e]); out["xbar0"].append(x0s[e] + PERTURB[name] * rng.standard_normal(n))
        out["Ubar"].append((us[e] + 0.1 * rng.standard_normal((HMAX, nu)))[:H])
        out["K"].append(0.1 * rng.standard_normal((HMAX, m, n))[:H]); out["kff"].append(0.1 * rng.standard_normal((HMAX, m))[:H])
        out["alpha"].append(1.0 if e == 0 else 0.0 if e == 1 else (e + 1.0) / (e + 3.0))
    res = {k: np.ascontiguousarray(np.stack(v, axis=1 if k in ("Ubar", "K", "kff") else 0)) for k, v in out.items()}
    if f32:
        res = {k: v.astype(np.float32).astype(np.float64) for k, v in res.items()}
    return res


def with_reference(inp, open_loop, f32=False):
    """adds Xbar [H+1,B,n] = open_loop(xbar0, Ubar): the open-loop trajectory from the perturbed start (rounded to fp32 for an fp32 handle)"""
    Xbar = np.asarray(open_loop(inp["xbar0"], inp["Ubar"]), dtype=np.float64)
    assert Xbar.shape == (inp["Ubar"].shape[0] + 1,) + inp["x0"].shape
    return dict(inp, Xbar=Xbar.astype(np.float32).astype(np.float64) if f32 else Xbar)


def law(inp, k, Xk, act_off, m, dtype=np.longdouble):
    """the control law of step k at the states Xk [B,n], in `dtype`; members of inp that are None count as the ABI says (Ubar: zeros, Xbar: zeros, K: zeros, kff: zeros,
    alpha: ones) -> (u [B,nu] in dtype, S [B,nu] = |Ubar| + |alpha kff| + sum_j |K_ij| |dx_j| on the driven inputs, |Ubar| elsewhere)"""
    T = lambda a: np.asarray(a, dtype=dtype)
    B, n = Xk.shape
    nu = n // 2
    Ub = T(inp["Ubar"][k]) if inp.get("Ubar") is not None else np.zeros((B, nu), dtype)
    dx = T(Xk) - (T(inp["Xbar"][k]) if (inp.get("Xbar") is not None and inp.get("K") is not None) else np.zeros((B, n), dtype))
    K = T(inp["K"][k]) if inp.get("K") is not None else np.zeros((B, m, n), dtype)
    kff = T(inp["kff"][k]) if inp.get("kff") is not None else np.zeros((B, m), dtype)
    alpha = T(inp["alpha"]) if inp.get("alpha") is not None else np.ones(B, dtype)
    fb = (K * dx[:, None, :]).sum(-1)
    u = Ub.copy(); u[:, act_off:act_off + m] += alpha[:, None] * kff + fb
    S = np.abs(Ub).copy(); S[:, act_off:act_off + m] += np.abs(alpha[:, None] * kff) + (np.abs(K) * np.abs(dx[:, None, :])).sum(-1)
    return u, S.astype(np.float64)


def gate(ref, S, n, f32):
    """per entry: (n + 4) 2^-53 S + 1/2 ulp_TIO(|ref|) -- the fp64 dot-product bound (n products and sums, the difference x - xbar, alpha kff and the sum with Ubar:
    n + 4 roundings of relative size 2^-53 on terms whose magnitudes add up to S) plus the one rounding to the ABI type"""
    tio = np.float32 if f32 else np.float64
    return (n + 4) * U53 * S + 0.5 * np.spacing(np.abs(np.asarray(ref, dtype=np.float64)).astype(tio)).astype(np.float64)
