"""Inputs and references shared by tests/test_sweep_options_gpu.py (the device) and tests/test_sweep_references.py (no device): the failure patterns of
the four reverse sweeps, the records with NaN Jacobians at the failed steps, state-space cotangents at quaternions that are not unit, and the recursions of
the four GPU test modules on them.  Nothing here touches the GPU; the four modules are imported for their helpers (synthetic, recursion, pull_back, check)."""
import numpy as np

import test_rollout_adjoint_gpu as O        # open-loop sweep
import test_policy_adjoint_gpu as P         # affine closed-loop sweep
import test_rollout_mlp_gpu as N            # network closed-loop sweep
import test_rollout_data_gpu as D           # contact-data sweep

U53, U23 = 2.0 ** -53, 2.0 ** -23

OPEN_MECHANISMS = ("pendulum", "fixed3", "ant")     # nx 12; no controls; nx 156
CLOSED_MECHANISMS = ("cartpole", "ant")
DATA_MECHANISMS = ("sphere", "ant")
HIDDEN = ([17, 5], [300])
FAILURE_SHAPES = ((4, 6), (1, 2))


def failure_status(H, B):
    """the status buffer of the failure tests.  (4, 6), one pattern per environment: 0 none; 1 the step that starts the sweep (k = H-1), status 1; 2 the step
    that ends it (k = 0), 1; 3 two steps in a row (k = 1, 2), 2; 4 every step, -1; 5 first and last (k = 0: -3, k = H-1: 7).  (1, 2): the only step of
    environment 1 (H = 1: first and last step at once).  (3, 5): the patterns of environments 1 and 2 alone."""
    st = np.zeros((H, B), np.int32)
    if (H, B) == (1, 2):
        st[0, 1] = 1
    elif (H, B) == (3, 5):
        st[H - 1, 1] = 1; st[0, 2] = 1
    elif (H, B) == (4, 6):
        st[H - 1, 1] = 1; st[0, 2] = 1; st[1:3, 3] = 2; st[:, 4] = -1; st[0, 5] = -3; st[H - 1, 5] = 7
    else:
        raise ValueError("no failure pattern for H = %d, B = %d" % (H, B))
    return st


def poisoned(a, status):
    """a copy of a Jacobian array [H,B,..] that is NaN at every failed (k, b)"""
    if a is None:
        return None
    a = a.copy(); a[status != 0] = np.nan
    return a


def limit(factor, abs_, ref, f32):
    """the bound of the four modules' check(): factor 2^-53 abs_ (+ 2^-23 |ref| for fp32 outputs), factor = 2 H (nx + extra) (open-loop, data) or
    2 (H n_step + n_red) (closed-loop)"""
    return factor * U53 * abs_ + (U23 * np.abs(ref) if f32 else 0.0)


def ratio(out, ref, lim):
    """max |out - ref| / lim over the entries with a positive bound (an entry whose bound is 0 is an exact zero of the reference: asserted elsewhere)"""
    err = np.abs(np.asarray(out, np.float64) - ref)
    ok = lim > 0
    return float((err[ok] / lim[ok]).max()) if ok.any() else 0.0


# ---------------------------------------------------------------- (a) failed steps ----------------------------------------------------------------
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def open_loop_failed(name, dtype, H, B):
    """-> dict: clean (DZ, DU, G), the poisoned DZ, DU, status, ref = (gU, gz) of O.recursion with the cut, abs = the same on magnitudes"""
    def make():
        DZ, DU, G = O.synthetic(name, dtype, H, B)
        st = failure_status(H, B)
        DZn, DUn = poisoned(DZ, st), poisoned(DU, st)
        return dict(clean=(DZ, DU, G), DZ=DZn, DU=DUn, G=G, status=st, ref=O.recursion(DZn, DUn, G, st),
                    abs=O.recursion(np.abs(DZ), None if DU is None else np.abs(DU), np.abs(G), st))
    return _once(("open", name, dtype, H, B), make)


def data_failed(name, dtype, H, B):
    """-> dict: clean (DZ, DC, G), the poisoned DZ, DC, status, ref = (a, gz) of D.recursion with the cut, abs = the same on magnitudes"""
    def make():
        DZ, DC, G = D.synthetic(name, dtype, H, B)
        st = failure_status(H, B)
        DZn, DCn = poisoned(DZ, st), poisoned(DC, st)
        return dict(clean=(DZ, DC, G), DZ=DZn, DC=DCn, G=G, status=st, ref=D.recursion(DZn, DCn, G, st), abs=D.recursion(np.abs(DZ), np.abs(DC), np.abs(G), st))
    return _once(("data", name, dtype, H, B), make)


def closed_loop_record(name, dtype, H, B, hidden=None, per_env=1):
    """the synthetic record of the affine sweep (hidden None) or of the network sweep, W / theta of environment 0 alone for a shared policy"""
    if hidden is None:
        inp = dict(P.synthetic(name, dtype, H, B)); key = "W"
    else:
        inp = dict(N.mlp_synthetic(name, dtype, H, B, hidden)); key = "theta"
    if not per_env:
        inp[key] = np.ascontiguousarray(inp[key][0])
    return inp


def closed_loop_failed(name, dtype, H, B, hidden=None, per_env=1):
    """-> (clean inputs, inputs with NaN DZ, DU at the failed steps and the status buffer); OBS, ACT, M, G, G_u, G_obs stay finite there"""
    clean = closed_loop_record(name, dtype, H, B, hidden, per_env)
    st = failure_status(H, B)
    return clean, dict(clean, DZ=poisoned(clean["DZ"], st), DU=poisoned(clean["DU"], st), status=st)


def closed_loop_recursion(name, inp, hidden=None, absolute=False):
    """the reference of the module the record belongs to (its per-environment outputs)"""
    spec = P._spec(name); act_off, na = P.ACT[name]
    if absolute:
        inp = P.absolute(inp)
    if hidden is None:
        return P.recursion(spec, inp, act_off, na, absolute=absolute)
    return N.recursion(spec, inp, act_off, N.widths_of(name, hidden), absolute=absolute)


def open_loop_zero(status):
    """where the open-loop and data recursions are exactly zero: gU[k, b] at every failed step, gz[b] (and so lambda) where step 0 failed"""
    return status != 0, status[0] != 0


# ---------------------------------------------------------------- (b), (c) state-space cotangents ----------------------------------------------------------------
def state_cotangents(spec, dtype, H, B, scaled=False, seed=11):
    """Z [H,B,13Nb] and state-space G [H,B,13Nb] as test_state_space_cotangents draws them (random unit quaternions, rounded to the dtype); scaled: every
    quaternion multiplied by a factor from [0.9, 1.1] before the rounding, so that an fp32 kernel that did not normalise would be off by up to 10 %"""
    rng = np.random.default_rng(seed); dt = np.float32 if dtype == "f32" else np.float64
    Z = rng.standard_normal((H, B, spec.Nb, 13))
    Z[..., 6:10] /= np.linalg.norm(Z[..., 6:10], axis=-1, keepdims=True)
    Gs = rng.standard_normal((H, B, spec.nz)).astype(dt)
    if scaled:
        Z[..., 6:10] *= np.random.default_rng(seed + 1000).uniform(0.9, 1.1, (H, B, spec.Nb, 1))
    return Z.reshape(H, B, spec.nz).astype(dt), Gs


def closed_loop_state_space(name, dtype, H, B, hidden=None, per_env=1, scaled=False, failed=False, normalise=None):
    """-> (device inputs with G in state coordinates and Z, reference inputs with G pulled back to tangent coordinates, the magnitude sums of the pull-back);
    normalise: what pull_back's f32 argument is (default: the dtype's own convention)"""
    spec = P._spec(name)
    inp = closed_loop_failed(name, dtype, H, B, hidden, per_env)[1] if failed else closed_loop_record(name, dtype, H, B, hidden, per_env)
    Z, Gs = state_cotangents(spec, dtype, H, B, scaled)
    Gt, Ga = O.pull_back(Gs, Z, dtype == "f32" if normalise is None else normalise)
    return dict(inp, G=Gs, Z=Z), dict(inp, G=Gt), Ga


def unnormalised_excess(kind, name, H, B, hidden=None):
    """the guard of the fp32 normalisation test: the reference that takes the scaled quaternions as given, measured against the bound around the reference
    that normalises them -> the largest |ref_given - ref_normalised| / bound over the sweep's outputs (a kernel without q / |q| would miss the bound by that factor)"""
    def make():
        worst = 0.0
        if kind in ("open", "data"):
            mod = O if kind == "open" else D
            spec = mod._spec(name); nx = spec.nx
            J0, J1, _ = mod.synthetic(name, "f32", H, B)
            Z, Gs = state_cotangents(spec, "f32", H, B, scaled=True)
            (Gn, Ga), (Gu, _) = O.pull_back(Gs, Z, True), O.pull_back(Gs, Z, False)
            rn, ru = mod.recursion(J0, J1, Gn), mod.recursion(J0, J1, Gu)
            ab = mod.recursion(np.abs(J0), None if J1 is None else np.abs(J1), Ga)
            for n_, u_, a_ in zip(rn, ru, ab):
                if n_.size:
                    worst = max(worst, ratio(u_, n_, limit(2.0 * H * (nx + (12 if kind == "open" else 13)), a_, n_, True)))
            return worst
        spec = P._spec(name); act_off, na = P.ACT[name]
        _, rin, Ga = closed_loop_state_space(name, "f32", H, B, hidden, scaled=True, normalise=True)
        _, uin, _ = closed_loop_state_space(name, "f32", H, B, hidden, scaled=True, normalise=False)
        rn, ru = closed_loop_recursion(name, rin, hidden), closed_loop_recursion(name, uin, hidden)
        ainp = dict(P.absolute(rin), G=Ga)
        ab = P.recursion(spec, ainp, act_off, na, absolute=True) if hidden is None else N.recursion(spec, ainp, act_off, N.widths_of(name, hidden), absolute=True)
        n_step = (spec.nx + 2 * spec.nu + na + 8 if hidden is None else N.n_step_of(spec, N.widths_of(name, hidden))) + 10
        for k in rn:
            worst = max(worst, ratio(ru[k], rn[k], limit(2.0 * H * n_step, ab[k], rn[k], True)))
        return worst
    return _once(("excess", kind, name, H, B, None if hidden is None else tuple(hidden)), make)
