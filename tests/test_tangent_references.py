"""The references of tests/test_rollout_tangent_gpu.py, pinned without a device: the forward recursion against the dense rollout Jacobian assembled block by
block, against the reverse recursions of the existing modules through the transpose identity, the push-forward against the pull-back, the failure table, and
the guard of the fp32 normalisation test."""
import numpy as np
import pytest

import sweep_cases as S
import tangent_cases as TC

O, D = S.O, S.D


def small_record(nx, nu, nth, H, B, seed):
    rng = np.random.default_rng(seed)
    DZ = 1.3 * rng.standard_normal((H, B, nx, nx)) / np.sqrt(nx)
    DU = rng.standard_normal((H, B, nu, nx)) if nu else None
    DC = rng.standard_normal((H, B, nth, nx)) if nth else None
    return DZ, DU, DC


# ---------------------------------------------------------------- (i) the dense rollout Jacobian ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["pendulum", "cartpole"])
def test_recursion_is_the_dense_rollout_jacobian(name):
    """dZ = J [dz0; dU_0 .. dU_{H-1}; dtheta] with J assembled block by block from A_k = DZ_k (rows r, columns c), B_k = DU_k, C_k = DC_k:
    block (k, z0) = A_k .. A_0,  (k, u_j) = A_k .. A_{j+1} B_j (j <= k),  (k, theta) = sum_{j <= k} A_k .. A_{j+1} C_j.  Five contact-data columns are drawn for
    both shapes (the mechanisms themselves have no contacts: the recursion does not know)."""
    spec = O._spec(name); nx, nu, nth = spec.nx, spec.nu, 5
    H, B, T = 3, 2, 3
    DZ, DU, DC = small_record(nx, nu, nth, H, B, 5)
    dz0, dU, dth = TC.tangents("f64", H, B, T, nx, nu, nth)
    out = TC.tangent_recursion(DZ, DU, DC, dz0, dU, dth)
    abs_ = TC.tangent_magnitudes(DZ, DU, DC, dz0, dU, dth)
    for b in range(B):
        A = [DZ[k, b].T for k in range(H)]; Bk = [DU[k, b].T for k in range(H)]; Ck = [DC[k, b].T for k in range(H)]
        J = np.zeros((H * nx, nx + H * nu + nth))
        for k in range(H):
            P = np.eye(nx)                                              # A_k .. A_{j+1}, j going down from k
            for j in range(k, -1, -1):
                J[k * nx:(k + 1) * nx, nx + j * nu:nx + (j + 1) * nu] = P @ Bk[j]
                J[k * nx:(k + 1) * nx, nx + H * nu:] += P @ Ck[j]
                P = P @ A[j]
            J[k * nx:(k + 1) * nx, :nx] = P
        for t in range(T):
            v = np.concatenate([dz0[b, t]] + [dU[k, b, t] for k in range(H)] + [dth[t]])
            want = (J @ v).reshape(H, nx)
            lim = TC.limit(H, nx + nu + nth, abs_[:, b, t], want, False)
            assert (np.abs(out[:, b, t] - want) <= lim).all() and np.abs(want).max() > 0.1


# ---------------------------------------------------------------- (ii) the transpose identity ----------------------------------------------------------------
def identity_sides(DZ, DU, DC, G, dz0, dU, dth, status):
    """per (b, t): <G, tangent(d)> and <reverse(G), d> with the reverse recursions of the open-loop and the data module; and the same on magnitudes"""
    def sides(DZ, DU, DC, G, dz0, dU, dth, rec):
        dZ = rec(DZ, DU, DC, dz0, dU, dth, status)
        lhs = np.einsum("kbr,kbtr->bt", G, dZ)
        gU, gz = O.recursion(DZ, DU, G, status)
        rhs = np.einsum("br,btr->bt", gz, dz0)
        if dU is not None:
            rhs = rhs + np.einsum("kbc,kbtc->bt", gU, dU)
        if dth is not None:
            a, _ = D.recursion(DZ, DC, G, status)
            rhs = rhs + np.einsum("bc,tc->bt", a, dth)
        return lhs, rhs
    (l, r) = sides(DZ, DU, DC, G, dz0, dU, dth, TC.tangent_recursion)
    ab = [None if a is None else np.abs(a) for a in (DZ, DU, DC, G, dz0, dU, dth)]
    (la, ra) = sides(*ab, TC.tangent_recursion)
    return l, r, la, ra


@pytest.mark.parametrize("failed", [False, True])
@pytest.mark.parametrize("name", ["cartpole", "sphere", "ant"])
def test_transpose_identity_of_the_references(name, failed):
    """<G, tangent(d)> = <O.recursion(G), (dz0, dU)> + <D.recursion(G), dtheta>, with and without failure_status(4, 6)"""
    H, B, T = 4, 6, 2
    data = name != "cartpole"
    DZ, DU, DC = TC.record(name, "f64", H, B, data=data)
    G = (D if data else O).synthetic(name, "f64", H, B)[2]
    nx = DZ.shape[2]; nu = 0 if DU is None else DU.shape[2]; nth = 0 if DC is None else DC.shape[2]
    assert G.shape == (H, B, nx)
    dz0, dU, dth = TC.tangents("f64", H, B, T, nx, nu, nth)
    st = S.failure_status(H, B) if failed else None
    if failed:
        DZ, DU, DC = S.poisoned(DZ, st), S.poisoned(DU, st), S.poisoned(DC, st)
    l, r, la, ra = identity_sides(DZ, DU, DC, G, dz0, dU, dth, st) if not failed else identity_sides_clean_magnitudes(name, H, B, data, G, dz0, dU, dth, st, DZ, DU, DC)
    lim = TC.identity_limit(H, nx, nu, nth, la, ra)
    assert np.isfinite(l).all() and np.isfinite(r).all()
    assert (np.abs(l - r) <= lim).all(), (np.abs(l - r) / lim).max()
    assert np.abs(l[0]).min() > 1e-3                                    # (environment 0 never fails: something is compared)
    if failed:
        assert (l[4] == 0).all() and (r[4] == 0).all()                  # environment 4: every step failed


def identity_sides_clean_magnitudes(name, H, B, data, G, dz0, dU, dth, st, DZn, DUn, DCn):
    """the values from the poisoned record, the magnitudes from the clean one (|NaN| has no use as a bound)"""
    l, r, _, _ = identity_sides(DZn, DUn, DCn, G, dz0, dU, dth, st)
    DZ, DU, DC = TC.record(name, "f64", H, B, data=data)
    _, _, la, ra = identity_sides(DZ, DU, DC, G, dz0, dU, dth, st)
    return l, r, la, ra


# ---------------------------------------------------------------- (iii) push-forward and pull-back ----------------------------------------------------------------
@pytest.mark.parametrize("scaled,f32", [(False, False), (True, True)])
def test_push_is_the_transpose_of_pull_back(scaled, f32):
    """<Gs, push(phi)> = <pull_back(Gs), phi> at unit quaternions and at quaternions scaled by up to 10 % with the fp32 rule (q / |q|)"""
    spec = O._spec("cartpole"); H, B, T = 2, 3, 2
    Z, Gs = S.state_cotangents(spec, "f64", H, B, scaled=scaled)
    phi = np.random.default_rng(23).standard_normal((H, B, T, spec.nx))
    ps, pa = TC.push(phi, Z, f32)
    gt, ga = O.pull_back(Gs, Z, f32)
    l = np.einsum("kbi,kbti->kbt", Gs, ps); r = np.einsum("kbi,kbti->kbt", gt, phi)
    mag = np.einsum("kbi,kbti->kbt", np.abs(Gs), pa)
    assert (np.abs(l - r) <= 4 * (spec.nz + 10) * S.U53 * mag).all()
    assert np.allclose(np.einsum("kbi,kbti->kbt", ga, np.abs(phi)), mag, rtol=1e-12)       # the magnitude sums are transposes of each other too
    # x, v, omega are copied; |dq| = |phi| at a unit quaternion
    t = phi.reshape(H, B, T, spec.Nb, 12); s = ps.reshape(H, B, T, spec.Nb, 13)
    assert np.array_equal(s[..., 0:6], t[..., 0:6]) and np.array_equal(s[..., 10:13], t[..., 9:12])
    assert np.allclose(np.linalg.norm(s[..., 6:10], axis=-1), np.linalg.norm(t[..., 6:9], axis=-1), rtol=1e-12)


# ---------------------------------------------------------------- (iv) the failure table ----------------------------------------------------------------
@pytest.mark.parametrize("hb", S.FAILURE_SHAPES)
def test_failure_table(hb):
    """exact zeros of dZ[k][b] at every failed (k, b), finite everywhere on NaN-poisoned records, and the tangent restarts behind a failed step when dU is given"""
    H, B = hb; T = 2
    DZ, DU, DC = TC.record("ant", "f64", H, B, data=True)
    nx, nu, nth = DZ.shape[2], DU.shape[2], DC.shape[2]
    st = S.failure_status(H, B)
    dz0, dU, dth = TC.tangents("f64", H, B, T, nx, nu, nth)
    for use in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        out = TC.tangent_recursion(S.poisoned(DZ, st), S.poisoned(DU, st), S.poisoned(DC, st), dz0 if use[0] else None, dU if use[1] else None, dth if use[2] else None, st)
        assert np.isfinite(out).all()
        assert (out[st != 0] == 0).all()
        ok_after_failure = np.zeros((H, B), bool)
        for k in range(1, H):
            ok_after_failure[k] = (st[k] == 0) & (st[k - 1] != 0)
        if ok_after_failure.any():
            restarted = np.abs(out[ok_after_failure]).max(axis=(-1, -2))
            assert (restarted > 0).all() if (use[1] or use[2]) else (restarted == 0).all()


# ---------------------------------------------------------------- the guard of the fp32 normalisation test ----------------------------------------------------------------
def unnormalised_excess(name, H, B, T):
    """the state-space reference that takes the scaled quaternions as given, measured against the bound around the one that normalises them"""
    spec = O._spec(name)
    DZ, DU, _ = TC.record(name, "f32", H, B)
    nu = 0 if DU is None else DU.shape[2]
    dz0, dU, _ = TC.tangents("f32", H, B, T, spec.nx, nu, 0)
    Z, _ = S.state_cotangents(spec, "f32", H, B, scaled=True)
    ref_t = TC.tangent_recursion(DZ, DU, None, dz0, dU, None); abs_t = TC.tangent_magnitudes(DZ, DU, None, dz0, dU, None)
    ref_n, abs_n = TC.push_bound_inputs(ref_t, abs_t, Z, True)
    ref_u, _ = TC.push(ref_t, Z, False)
    return S.ratio(ref_u, ref_n, TC.limit(H, spec.nx + nu, abs_n, ref_n, True, extra=2 + TC.PUSH_EXTRA))


def test_unnormalised_reference_misses_the_bound():
    """the device test of tan_space = 1 in fp32 can tell: a kernel that did not use q / |q| would miss its bound by this factor"""
    excess = unnormalised_excess("cartpole", 3, 5, 2)
    print("state-space tangents without q / |q|: %.0f x the bound" % excess)
    assert excess > 100.0
