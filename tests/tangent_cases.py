"""Inputs and references shared by tests/test_rollout_tangent_gpu.py (the device) and tests/test_tangent_references.py (no device): the forward recursion of
dojo_rollout_tangent_dev in fp64 NumPy, its twin on magnitudes, the push-forward to state coordinates, the records and tangents the device tests draw.  Nothing
here touches the GPU; the modules of the reverse sweeps are imported for their helpers (synthetic, recursion, pull_back, _spec).

The recursion, per environment b and tangent t:
    delta <- dz0[b][t];   for k = 0 .. H-1:  failed step: delta <- 0;  else delta <- DZ_k delta + DU_k dU[k][b][t] + DC_k dtheta[t];   dZ[k][b][t] <- delta

Error bound (elementwise, the project's own: tests/test_rollout_adjoint_gpu.py): every output is a chain of at most H sums of at most n = nx + nu + 5Nc products,
all in fp64; two summation orders of such a sum differ by at most gamma_n sum |x_i y_i| each, so with `abs_` the same recursion on magnitudes
    |out - ref| <= 2 H (n + 2) 2^-53 abs_   (+ 2^-23 |ref| for fp32 outputs: one rounding of the result)
and (n + 2 + 10) where the tangent is then pushed forward to state coordinates (the ten operations of the quaternion product, as for the pulled-back cotangents)."""
import numpy as np

import sweep_cases as S

O, D = S.O, S.D
U53, U23 = S.U53, S.U23
PUSH_EXTRA = 10


def tangent_recursion(DZ, DU, DC, dz0, dU, dth, status=None):
    """the reference: fp64 NumPy.  DZ [H,B,c,r], DU [H,B,nu,r] or None, DC [H,B,nth,r] or None, dz0 [B,T,nx] or None, dU [H,B,T,nu] or None, dth [T,nth] or None
    -> dZ [H,B,T,nx].  A failed step's Jacobians are not touched."""
    H, B, nx = DZ.shape[:3]
    T = [a.shape[i] for a, i in ((dz0, 1), (dU, 2), (dth, 0)) if a is not None][0]
    delta = np.zeros((B, T, nx)) if dz0 is None else np.asarray(dz0, np.float64).copy()
    out = np.zeros((H, B, T, nx))
    for k in range(H):
        ok = np.ones(B, bool) if status is None else (status[k] == 0)
        new = np.zeros((B, T, nx))
        new[ok] = np.einsum("bcr,btc->btr", np.asarray(DZ[k][ok], np.float64), delta[ok])
        if dU is not None:
            new[ok] += np.einsum("bcr,btc->btr", np.asarray(DU[k][ok], np.float64), np.asarray(dU[k][ok], np.float64))
        if dth is not None:
            new[ok] += np.einsum("bcr,tc->btr", np.asarray(DC[k][ok], np.float64), np.asarray(dth, np.float64))
        delta = new
        out[k] = delta
    return out


def _abs(a):
    return None if a is None else np.abs(np.asarray(a, np.float64))


def tangent_magnitudes(DZ, DU, DC, dz0, dU, dth, status=None):
    """the magnitude twin: the same recursion on |.| -> abs_ of the bound"""
    return tangent_recursion(_abs(DZ), _abs(DU), _abs(DC), _abs(dz0), _abs(dU), _abs(dth), status)


def n_terms(DZ, dU, dth):
    """nx + nu + 5Nc of the bound: the columns that are swept"""
    return DZ.shape[2] + (0 if dU is None else dU.shape[3]) + (0 if dth is None else dth.shape[1])


def limit(H, n, abs_, ref, f32, extra=2):
    return S.limit(2.0 * H * (n + extra), abs_, ref, f32)


def check(out, ref, abs_, H, n, f32, extra=2, what=""):
    """out finite and within the bound of ref; prints the largest error / bound"""
    lim = limit(H, n, abs_, ref, f32, extra)
    err = np.abs(np.asarray(out, np.float64) - ref)
    assert np.isfinite(out).all(), what
    print("%s: max error %.3e, largest error / bound %.3f" % (what, err.max(), S.ratio(out, ref, lim)))
    worst = (err - lim).max()
    assert worst <= 0.0, "%s: error exceeds the bound by %.3e (max error %.3e, max |ref| %.3e)" % (what, worst, err.max(), np.abs(ref).max())


def identity_limit(H, nx, nu, nth, la, ra, f32=False):
    """The tolerance of the transpose identity <G, tangent(d)> = <reverse(G), d>: both sides' rounding bounds added.  Each side is its recursion's bound
    contracted with the magnitudes of the other factor -- both contractions are the same number, the identity on magnitudes (la = ra up to rounding: the larger
    is taken) -- plus one dot product each, of H nx terms on the left and of nx + H nu + 5Nc on the right.  fp32 outputs: one rounding of every number a device
    wrote, 2^-23 per side."""
    n = nx + nu + nth
    s = np.maximum(la, ra)
    return (2 * 2.0 * H * (n + 2) + 2.0 * (H * nx + nx + H * nu + nth)) * U53 * s + (2 * U23 * s if f32 else 0.0)


def push(dZt, Z, f32):
    """tangent [H,B,T,12Nb] -> state [H,B,T,13Nb] at the states Z [H,B,13Nb]: x, v, omega copied, dq = q (x) (0, phi) (f32: at q / |q|); and the sum of the
    magnitudes of the terms of every entry"""
    from dojo_amd import quat
    H, B, T, nx = dZt.shape
    Nb = nx // 12
    t = np.asarray(dZt, np.float64).reshape(H, B, T, Nb, 12)
    q = np.asarray(Z, np.float64).reshape(H, B, 1, Nb, 13)[..., 6:10]
    if f32:
        q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    q = np.moveaxis(np.broadcast_to(q, (H, B, T, Nb, 4)), -1, 0)
    phi = np.moveaxis(t[..., 6:9], -1, 0)
    dq = np.moveaxis(quat.qmul(q, np.concatenate([np.zeros((1,) + phi.shape[1:]), phi])), 0, -1)
    aq, ap = np.abs(q), np.abs(phi)
    adq = np.stack([aq[1] * ap[0] + aq[2] * ap[1] + aq[3] * ap[2]]
                   + [aq[0] * ap[a] + aq[1 + (a + 1) % 3] * ap[(a + 2) % 3] + aq[1 + (a + 2) % 3] * ap[(a + 1) % 3] for a in range(3)], -1)
    s = np.concatenate([t[..., 0:6], dq, t[..., 9:12]], -1).reshape(H, B, T, 13 * Nb)
    sa = np.concatenate([np.abs(t[..., 0:6]), adq, np.abs(t[..., 9:12])], -1).reshape(H, B, T, 13 * Nb)
    return s, sa


def push_bound_inputs(ref_t, abs_t, Z, f32):
    """(reference, abs_) of a state-space output: the pushed reference, and the push of the tangent-space magnitudes (its magnitude sums)"""
    ref_s, _ = push(ref_t, Z, f32)
    _, abs_s = push(abs_t, Z, f32)
    return ref_s, abs_s


# ---------------------------------------------------------------- the cases of the device tests ----------------------------------------------------------------
_cache = {}


def record(name, dtype, H, B, data=False):
    """(DZ, DU, DC) in the dtype.  data = False: the open-loop module's record (O.synthetic; DC None).  data = True: the data module's DZ and DC (D.synthetic),
    and DU ~ N(0,1) drawn here for mechanisms with inputs"""
    key = ("record", name, dtype, H, B, data)
    if key not in _cache:
        if not data:
            DZ, DU, _ = O.synthetic(name, dtype, H, B)
            _cache[key] = (DZ, DU, None)
        else:
            DZ, DC, _ = D.synthetic(name, dtype, H, B)
            nu = D._spec(name).nu
            DU = np.random.default_rng(41).standard_normal((H, B, nu, DZ.shape[2])).astype(DZ.dtype) if nu else None
            _cache[key] = (DZ, DU, DC)
    return _cache[key]


def tangents(dtype, H, B, T, nx, nu, nth, seed=17):
    """dz0 [B,T,nx], dU [H,B,T,nu] or None, dth [T,nth] or None ~ N(0,1) in the dtype.  Tangent t of a draw with T' > T tangents is tangent t of the draw with T
    (each tangent has its own stream), so that the bit-identity tests can run one direction alone or among others"""
    dt = np.float32 if dtype == "f32" else np.float64
    dz0 = np.empty((B, T, nx), dt); dU = np.empty((H, B, T, nu), dt) if nu else None; dth = np.empty((T, nth), dt) if nth else None
    for t in range(T):
        rng = np.random.default_rng([seed, t])
        dz0[:, t] = rng.standard_normal((B, nx))
        if nu:
            dU[:, :, t] = rng.standard_normal((H, B, nu))
        if nth:
            dth[t] = rng.standard_normal(nth)
    return dz0, dU, dth
