"""The references and inputs of tests/test_sweep_options_gpu.py, pinned without a device: pull_back against an explicit matrix, the failure patterns
against the table they were specified with, the recursions on records with NaN Jacobians at the failed steps (finite, and non-zero wherever the device test
compares something that is not claimed to be zero), and the guard of the fp32 normalisation test."""
import numpy as np
import pytest

import sweep_cases as S

O, P, N, D = S.O, S.P, S.N, S.D


# ---------------------------------------------------------------- pull_back ----------------------------------------------------------------
def L_of(q):
    """left multiplication matrix: q (x) p = L(q) p, scalar first"""
    s, x, y, z = q
    return np.array([[s, -x, -y, -z], [x, s, -z, y], [y, z, s, -x], [z, -y, x, s]])


VT = np.vstack([np.zeros((1, 3)), np.eye(3)])       # the 4x3 V^T: phi -> (0, phi)


@pytest.mark.parametrize("module", [O, D], ids=["open_loop", "data"])
def test_pull_back_is_the_attitude_jacobian_transposed(module):
    """dq = q (x) (0, phi) = L(q) V^T phi, so g_phi = (L(q) V^T)^T g_q; x, v, omega are copied.  f32 = True is the same at q / |q|."""
    rng = np.random.default_rng(3)
    H, B, Nb = 2, 3, 4
    Z = rng.standard_normal((H, B, Nb, 13)); Gs = rng.standard_normal((H, B, Nb, 13))
    Z[..., 6:10] /= np.linalg.norm(Z[..., 6:10], axis=-1, keepdims=True)
    for scaled, f32 in ((False, False), (True, True)):
        Zs = Z.copy()
        if scaled:
            Zs[..., 6:10] *= rng.uniform(0.9, 1.1, (H, B, Nb, 1))
        t, ta = module.pull_back(Gs.reshape(H, B, -1), Zs.reshape(H, B, -1), f32)
        t = t.reshape(H, B, Nb, 12); ta = ta.reshape(H, B, Nb, 12)
        for idx in np.ndindex(H, B, Nb):
            q = Z[idx][6:10]                                            # the unit quaternion: what f32 = True must recover from the scaled one
            g = Gs[idx]
            want = np.concatenate([g[0:6], (L_of(q) @ VT).T @ g[6:10], g[10:13]])
            assert np.abs(t[idx] - want).max() <= 1e-14 * max(1.0, np.abs(want).max())
            mag = np.concatenate([np.abs(g[0:6]), np.abs(L_of(q) @ VT).T @ np.abs(g[6:10]), np.abs(g[10:13])])
            assert np.abs(ta[idx] - mag).max() <= 1e-14 * max(1.0, mag.max())
    # without the normalisation a scaled quaternion scales g_phi
    Zs = Z.copy(); Zs[..., 6:10] *= 1.1
    t0 = O.pull_back(Gs.reshape(H, B, -1), Z.reshape(H, B, -1), False)[0].reshape(H, B, Nb, 12)
    t1 = O.pull_back(Gs.reshape(H, B, -1), Zs.reshape(H, B, -1), False)[0].reshape(H, B, Nb, 12)
    assert np.allclose(t1[..., 6:9], 1.1 * t0[..., 6:9], rtol=0.0, atol=1e-13) and np.array_equal(t1[..., 0:6], t0[..., 0:6])


# ---------------------------------------------------------------- the pattern table ----------------------------------------------------------------
def test_failure_patterns_are_the_specified_table():
    H, B = 4, 6
    st = S.failure_status(H, B)
    assert st.dtype == np.int32 and st.shape == (H, B)
    table = {0: {}, 1: {H - 1: 1}, 2: {0: 1}, 3: {1: 2, 2: 2}, 4: {0: -1, 1: -1, 2: -1, 3: -1}, 5: {0: -3, H - 1: 7}}
    for b, failed in table.items():
        for k in range(H):
            assert st[k, b] == failed.get(k, 0), (k, b)
    bad = st != 0
    assert not bad[:, 0].any()                                          # an untouched environment
    assert bad[H - 1, 1] and not bad[:H - 1, 1].any()                   # the step that starts the sweep, alone
    assert bad[0, 2] and not bad[1:, 2].any()                           # the step that ends it, alone
    assert any(bad[k, b] and bad[k - 1, b] and not bad[:, b].all() for b in range(B) for k in range(1, H))      # two in a row, between solved steps
    assert bad[:, 4].all()                                              # every step
    assert bad[0, 5] and bad[H - 1, 5] and not bad[1:H - 1, 5].any()    # first and last, solved steps between
    assert set(np.unique(st[bad])) == {1, 2, -1, -3, 7}                 # "any non-zero": positive, negative, more than one bit
    one = S.failure_status(1, 2)
    assert one.shape == (1, 2) and one[0, 0] == 0 and one[0, 1] == 1    # H = 1: the first step is the last
    two = S.failure_status(3, 5)
    assert np.array_equal(np.argwhere(two != 0), [[0, 2], [2, 1]])      # the patterns of environments 1 and 2 at H = 3
    assert S.FAILURE_SHAPES == ((4, 6), (1, 2))


def test_poisoned_is_nan_at_the_failed_steps_only():
    st = S.failure_status(4, 6)
    a = np.ones((4, 6, 3, 2))
    p = S.poisoned(a, st)
    assert np.isnan(p[st != 0]).all() and (p[st == 0] == 1.0).all() and (a == 1.0).all() and S.poisoned(None, st) is None


# ---------------------------------------------------------------- the recursions on the failure inputs ----------------------------------------------------------------
def nonzero_rows(a):
    """per leading index: does the block hold a non-zero entry"""
    return np.abs(a.reshape(a.shape[0], -1)).max(1) > 0 if a.size else np.zeros(a.shape[0], bool)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("hb", S.FAILURE_SHAPES)
@pytest.mark.parametrize("name", S.OPEN_MECHANISMS)
def test_open_loop_reference_on_the_failure_inputs(name, hb, dtype):
    H, B = hb
    c = S.open_loop_failed(name, dtype, H, B)
    st = c["status"]; bad = st != 0
    assert np.isnan(c["DZ"][bad]).all() and (c["DU"] is None or np.isnan(c["DU"][bad]).all())
    rU, rz = c["ref"]; aU, az = c["abs"]
    assert np.isfinite(rU).all() and np.isfinite(rz).all() and np.isfinite(aU).all() and np.isfinite(az).all()
    zU, zz = S.open_loop_zero(st)
    assert np.array_equal(nonzero_rows(rz), ~zz)                         # gz: zero exactly where step 0 failed
    if rU.shape[2]:
        assert np.array_equal(np.abs(rU).max(2) > 0, ~zU)               # gU[k, b]: zero exactly at the failed steps
    assert (az >= np.abs(rz)).all() and (aU >= np.abs(rU)).all()
    if (H, B) == (4, 6):
        assert zz[4] and zU[:, 4].all()                                 # environment 4: nothing at all


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("hb", S.FAILURE_SHAPES)
@pytest.mark.parametrize("name", S.DATA_MECHANISMS)
def test_data_reference_on_the_failure_inputs(name, hb, dtype):
    H, B = hb
    c = S.data_failed(name, dtype, H, B)
    st = c["status"]; bad = st != 0
    assert np.isnan(c["DZ"][bad]).all() and np.isnan(c["DC"][bad]).all()
    ra, rz = c["ref"]; aa, az = c["abs"]
    assert np.isfinite(ra).all() and np.isfinite(rz).all() and np.isfinite(aa).all() and np.isfinite(az).all()
    assert np.array_equal(nonzero_rows(rz), st[0] == 0)                  # gz: zero exactly where step 0 failed
    assert np.array_equal(nonzero_rows(ra), ~bad.all(0))                 # gtheta_env: zero exactly where every step failed
    assert np.abs(D.batch_sum(ra)).min() > 0                             # the shared sum: every entry non-zero
    assert (aa >= np.abs(ra)).all() and (az >= np.abs(rz)).all()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("hb", S.FAILURE_SHAPES)
@pytest.mark.parametrize("name,hidden", [(m, h) for m in S.CLOSED_MECHANISMS for h in (None,) + S.HIDDEN], ids=lambda v: str(v).replace(" ", ""))
def test_closed_loop_reference_on_the_failure_inputs(name, hidden, hb, dtype):
    """affine (hidden None) and network sweeps, per environment and shared: OBS, ACT, M, G, G_u, G_obs are finite at the failed steps -- the kernels read them
    there -- and every per-environment output block is non-zero (the control cotangent and the feedback through M reach every step)"""
    H, B = hb
    for per_env in (1, 0):
        clean, bad = S.closed_loop_failed(name, dtype, H, B, hidden, per_env)
        st = bad["status"]; f = st != 0
        assert np.isnan(bad["DZ"][f]).all() and np.isnan(bad["DU"][f]).all()
        for k in ("OBS", "G", "G_u", "G_obs") + (("ACT",) if hidden else ()):
            assert np.isfinite(bad[k]).all(), k
        ref = S.closed_loop_recursion(name, bad, hidden); abs_ = S.closed_loop_recursion(name, bad, hidden, absolute=True)
        for k, v in ref.items():
            assert np.isfinite(v).all() and np.isfinite(abs_[k]).all(), k
            assert (abs_[k] >= np.abs(v)).all(), k
            if k == "gU":
                assert (np.abs(v).max(2) > 0).all()
                assert np.array_equal(v[f], np.asarray(bad["G_u"], np.float64)[f])      # a failed step's gU is the control cotangent alone
            else:
                assert nonzero_rows(v).all(), k
                if not per_env:
                    assert np.abs(v.sum(0)).max() > 0, k


# ---------------------------------------------------------------- the guard of the fp32 normalisation test ----------------------------------------------------------------
@pytest.mark.parametrize("kind,name,hidden", [("open", "ant", None), ("data", "ant", None), ("policy", "ant", None), ("mlp", "ant", [17, 5])], ids=["open", "data", "policy", "mlp"])
def test_unnormalised_reference_misses_the_bound(kind, name, hidden):
    """quaternions scaled by factors from [0.9, 1.1]: the reference that takes them as given is at least 100 bounds away from the one that normalises"""
    worst = S.unnormalised_excess(kind, name, 3, 5, hidden)
    print("%s: the un-normalised reference is %.3e bounds away" % (kind, worst))
    assert worst >= 100.0
    spec = P._spec(name)
    Z, _ = S.state_cotangents(spec, "f32", 3, 5, scaled=True)
    n = np.linalg.norm(Z.reshape(3, 5, spec.Nb, 13)[..., 6:10].astype(np.float64), axis=-1)
    assert n.min() >= 0.9 - 1e-6 and n.max() <= 1.1 + 1e-6 and np.abs(n - 1.0).max() > 0.05
    Zu, _ = S.state_cotangents(spec, "f32", 3, 5)
    assert np.abs(np.linalg.norm(Zu.reshape(3, 5, spec.Nb, 13)[..., 6:10].astype(np.float64), axis=-1) - 1.0).max() < 2e-7     # (the existing inputs: unit to rounding)
