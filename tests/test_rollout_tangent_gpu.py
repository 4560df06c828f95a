"""Forward-mode rollouts on the GPU: dojo_rollout_tangent_dev against the recursion it implements (tests/tangent_cases.py, pinned on the CPU by
tests/test_tangent_references.py), against the existing reverse sweeps through the transpose identity, its failure rule, state-space output, bit identity
across T, B and runs, optional inputs, argument errors; then real rollouts (central differences, the forward chain over the record's own Jacobians), the
host entry end to end, and the Gauss-Newton path of the sphere example.

The bound of every comparison is the one of tests/tangent_cases.py: 2 H (nx + nu + 5Nc + 2) 2^-53 abs_ (+ 2^-23 |ref| for fp32 outputs)."""
import os
import sys

import numpy as np
import pytest
import torch

import dojo_amd as d
from dojo_amd import api
from gpu_util import dev, guarded, guards_intact, tdt_of

import sweep_cases as S
import tangent_cases as TC

pytestmark = pytest.mark.gpu

O, D = S.O, S.D
INVALID, UNSUPPORTED = -1, -2
def teardown_module(module):
    """the handles live in the two modules' caches (whose own teardown may have run already)"""
    for mod in (O, D):
        for gm in mod._handles.values():
            gm.close()
        mod._handles.clear()


def tangent_raw(gm, H, T, DZ, DU, DC, dz0, dU, dth, tan_space=0, Z=None, status=None, dZ=None):
    """dojo_rollout_tangent_dev on torch tensors (None = NULL) -> return code"""
    return api.lib().dojo_rollout_tangent_dev(gm.h, int(H), int(T), api.addr(DZ), api.addr(DU), api.addr(DC), api.addr(dz0), api.addr(dU), api.addr(dth), int(tan_space), api.addr(Z), api.addr(status),
                                              api.addr(dZ), api.torch_stream())


def sweep(gm, rec, tans, tan_space=0, Z=None, status=None, raw=False):
    """NumPy in: rec = (DZ, DU, DC), tans = (dz0, dU, dth), None = NULL.  -> dZ [H,B,T,nx or 13Nb] (NumPy; raw: the device tensor).  The output starts as NaN between
    guard elements, which must come back untouched."""
    DZ, DU, DC = rec; dz0, dU, dth = tans
    H, B = DZ.shape[:2]
    T = [a.shape[i] for a, i in ((dz0, 1), (dU, 2), (dth, 0)) if a is not None][0]
    out = guarded((H, B, T, gm.spec.nz if tan_space else gm.spec.nx), tdt_of(gm))
    keep = [dev(a) for a in (DZ, DU, DC, dz0, dU, dth, Z, status)]
    api._chk(tangent_raw(gm, H, T, *keep[:6], tan_space, keep[6], keep[7], out))
    torch.cuda.synchronize()
    assert guards_intact(out)
    return out if raw else out.cpu().numpy()


def dims(rec):
    DZ, DU, DC = rec
    return DZ.shape[2], (0 if DU is None else DU.shape[2]), (0 if DC is None else DC.shape[2])


def compare(gm, rec, tans, H, f32, what, status=None):
    """the device against the recursion on the same values, with the module's bound"""
    out = sweep(gm, rec, tans, status=status)
    ref = TC.tangent_recursion(*rec, *tans, status)
    abs_ = TC.tangent_magnitudes(*rec, *tans, status) if status is None else TC.tangent_magnitudes(*clean_of(rec), *tans, status)
    TC.check(out, ref, abs_, H, TC.n_terms(rec[0], tans[1], tans[2]), f32, what=what)
    return out, ref


_clean = {}


def clean_of(rec):
    """the record a poisoned one was made from (|NaN| has no use in a bound)"""
    return _clean.get(id(rec[0]), rec)


def poisoned_record(rec, st):
    out = tuple(S.poisoned(a, st) for a in rec)
    _clean[id(out[0])] = rec
    return out


# ---------------------------------------------------------------- 1. kernel = recursion ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,hb", O.CASES)
def test_kernel_matches_the_recursion(name, hb, dtype):
    """synthetic records, no solver involved: nx = 12 (one body: three or six pieces per column, sixteen teams), 36 without controls (DU / dU NULL), 24, 156 (39
    pieces: six teams, lanes left over; pieces that end inside a 16-lane row), 372 (two teams in fp32, one in fp64).  T = 1, 4, 5: a padded chunk, a full one,
    two chunks; 9 (three chunks) on ant (2, 3)."""
    H, B = hb
    gm = O._handle(name, dtype, B); nx, nu = gm.spec.nx, gm.spec.nu
    rec = TC.record(name, dtype, H, B)
    assert (rec[1] is None) == (nu == 0)
    for T in (1, 4, 5) + ((9,) if (name, hb) == ("ant", (2, 3)) else ()):
        dz0, dU, _ = TC.tangents(dtype, H, B, T, nx, nu, 0)
        compare(gm, rec, (dz0, dU, None), H, dtype == "f32", "%s T=%d" % (name, T))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,hb", D.CASES)
def test_kernel_matches_the_recursion_with_contact_data(name, hb, dtype):
    """the data columns: sphere (5 columns: fewer than one item), block (20), ant (20 behind 156 + nu), atlas; all three inputs at once"""
    H, B = hb
    gm = D._handle(name, dtype, B); nx, nu, nth = gm.spec.nx, gm.spec.nu, 5 * len(gm.spec.contacts)
    rec = TC.record(name, dtype, H, B, data=True)
    assert dims(rec) == (nx, nu, nth) and nth > 0
    for T in (1, 4, 5):
        compare(gm, rec, TC.tangents(dtype, H, B, T, nx, nu, nth), H, dtype == "f32", "%s T=%d" % (name, T))


# ---------------------------------------------------------------- 2. the transpose identity, on the device ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,hb,failed", [("ant", (7, 65), False), ("sphere", (7, 65), False), ("ant", (4, 6), True), ("sphere", (4, 6), True)])
def test_transpose_identity_against_the_adjoint_kernels(name, hb, failed, dtype):
    """sum_k <G_k, dZ_k> = <gz, dz0> + sum_k <gU_k, dU_k> + <gtheta_env[b], dtheta> per environment and tangent: the forward sweep against
    dojo_rollout_adjoint_dev and dojo_rollout_data_adjoint_dev over the same record, no NumPy recursion in between (the magnitudes of the tolerance alone are
    NumPy's).  With a status buffer the two sides also have to agree about what a failed step does."""
    H, B = hb; T = 2; f32 = dtype == "f32"
    gm = D._handle(name, dtype, B); nx, nu, nth = gm.spec.nx, gm.spec.nu, 5 * len(gm.spec.contacts)
    clean = TC.record(name, dtype, H, B, data=True)
    G = D.synthetic(name, dtype, H, B)[2]
    st = S.failure_status(H, B) if failed else None
    rec = poisoned_record(clean, st) if failed else clean
    tans = TC.tangents(dtype, H, B, T, nx, nu, nth)
    dZ = sweep(gm, rec, tans, status=st).astype(np.float64)
    gU, gz = O.adjoint(gm, rec[0], rec[1], G, status=st)
    gte, _, gz2 = D.data_adjoint(gm, rec[0], rec[2], G, status=st, want=("env", "gz"))
    assert np.array_equal(gz, gz2)
    G64 = G.astype(np.float64)
    lhs = np.einsum("kbr,kbtr->bt", G64, dZ)
    rhs = np.einsum("br,btr->bt", gz.astype(np.float64), tans[0].astype(np.float64)) + np.einsum("bc,tc->bt", gte.astype(np.float64), tans[2].astype(np.float64))
    if nu:
        rhs = rhs + np.einsum("kbc,kbtc->bt", gU.astype(np.float64), tans[1].astype(np.float64))
    s = np.einsum("kbr,kbtr->bt", np.abs(G64), TC.tangent_magnitudes(*clean, *tans, st))
    lim = TC.identity_limit(H, nx, nu, nth, s, s, f32)
    print("%s %s failed=%s: largest |lhs - rhs| / tolerance = %.3f" % (name, dtype, failed, S.ratio(lhs, rhs, lim)))
    assert np.isfinite(lhs).all() and np.isfinite(rhs).all()
    assert (np.abs(lhs - rhs) <= lim).all()
    assert np.abs(lhs[0]).max() > 1e-3                                  # (environment 0 never fails: something is compared)
    if failed:
        assert (lhs[4] == 0).all() and (rhs[4] == 0).all()              # environment 4: every step failed


# ---------------------------------------------------------------- 3. failed steps ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("hb", S.FAILURE_SHAPES)
def test_nothing_flows_through_a_failed_step(hb, dtype):
    """records that are NaN at the failed steps: outputs finite, exactly zero at every failed (k, b), within the bound elsewhere; the tangent restarts behind a
    failed step when dU is given, and stays zero when only dz0 is"""
    H, B = hb; T = 5
    gm = D._handle("ant", dtype, B); nx, nu, nth = gm.spec.nx, gm.spec.nu, 5 * len(gm.spec.contacts)
    st = S.failure_status(H, B)
    rec = poisoned_record(TC.record("ant", dtype, H, B, data=True), st)
    dz0, dU, dth = TC.tangents(dtype, H, B, T, nx, nu, nth)
    after = np.zeros((H, B), bool)
    for k in range(1, H):
        after[k] = (st[k] == 0) & (st[k - 1] != 0)
    for tans, restarts in (((dz0, dU, dth), True), ((dz0, dU, None), True), ((dz0, None, None), False)):
        out, ref = compare(gm, rec, tans, H, dtype == "f32", "failed steps", status=st)
        assert (out[st != 0] == 0).all()
        if after.any():
            mag = np.abs(out[after]).max(axis=(-1, -2))
            assert (mag > 0).all() if restarts else (mag == 0).all()
    # a status buffer of zeros is no status buffer
    clean = clean_of(rec)
    a = sweep(gm, clean, (dz0, dU, dth), status=np.zeros((H, B), np.int32), raw=True); b = sweep(gm, clean, (dz0, dU, dth), raw=True)
    assert torch.equal(a, b)


# ---------------------------------------------------------------- 4. state-space output ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["cartpole", "ant"])
def test_state_space_tangents(name, dtype):
    """tan_space = 1 against push(tangent_recursion); fp32 with quaternions up to 10 % off unit (the kernel uses q / |q|: a reference that does not misses the
    bound by more than 100 x, tests/test_tangent_references.py).  Then with failed steps whose states are NaN: zeros there, nothing read."""
    H, B, T = 3, 5, 5; f32 = dtype == "f32"
    gm = O._handle(name, dtype, B); nx, nu = gm.spec.nx, gm.spec.nu
    rec = TC.record(name, dtype, H, B)
    tans = TC.tangents(dtype, H, B, T, nx, nu, 0)[:2] + (None,)
    Z, _ = S.state_cotangents(gm.spec, dtype, H, B, scaled=f32)
    for st in (None, S.failure_status(H, B)):
        r = rec if st is None else poisoned_record(rec, st)
        Zs = Z if st is None else S.poisoned(Z, st)
        out = sweep(gm, r, tans, tan_space=1, Z=Zs, status=st)
        ref_t = TC.tangent_recursion(*r, *tans, st); abs_t = TC.tangent_magnitudes(*rec, *tans, st)
        ref_s, abs_s = TC.push_bound_inputs(ref_t, abs_t, Z, f32)
        TC.check(out, ref_s, abs_s, H, nx + nu, f32, extra=2 + TC.PUSH_EXTRA, what="%s state space%s" % (name, "" if st is None else ", failed steps"))
        if st is not None:
            assert (out[st != 0] == 0).all()


# ---------------------------------------------------------------- 5. bit identity ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_bit_identical_across_T_B_and_runs(dtype):
    """fixed summation order: a tangent's result does not depend on T or on its slot (alone, among 5, among 9 -- the last of three chunks), an environment's not
    on B or on its place (alone against 0, 32, 64 of 65), and two runs agree"""
    H, B = 7, 65
    gm = D._handle("ant", dtype, B); nx, nu, nth = gm.spec.nx, gm.spec.nu, 5 * len(gm.spec.contacts)
    rec = TC.record("ant", dtype, H, B, data=True)
    t9 = TC.tangents(dtype, H, B, 9, nx, nu, nth)
    pick = lambda tans, sl: (tans[0][:, sl], tans[1][:, :, sl], tans[2][sl])
    o9 = sweep(gm, rec, t9, raw=True)
    assert torch.equal(o9, sweep(gm, rec, t9, raw=True))
    o5 = sweep(gm, rec, pick(t9, slice(0, 5)), raw=True)
    assert torch.equal(o5, o9[:, :, :5])
    for t in (0, 4, 8):
        o1 = sweep(gm, rec, pick(t9, slice(t, t + 1)), raw=True)
        assert torch.equal(o1[:, :, 0], o9[:, :, t]), t
    g1 = D._handle("ant", dtype, 1)
    for b in (0, 32, 64):
        ob = sweep(g1, tuple(a[:, b:b + 1] for a in rec), (t9[0][b:b + 1], t9[1][:, b:b + 1], t9[2]), raw=True)
        assert torch.equal(ob[:, 0], o9[:, b]), b


# ---------------------------------------------------------------- 6. optional inputs and guards ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_optional_inputs(dtype):
    """each of dz0, dU, dtheta absent alone and in pairs; the Jacobian array of an absent input NULL in one call and all NaN in another: never read.  (sweep()
    checks the guard elements around the output on every call.)"""
    H, B, T = 2, 3, 5
    gm = D._handle("ant", dtype, B); nx, nu, nth = gm.spec.nx, gm.spec.nu, 5 * len(gm.spec.contacts)
    DZ, DU, DC = TC.record("ant", dtype, H, B, data=True)
    dz0, dU, dth = TC.tangents(dtype, H, B, T, nx, nu, nth)
    full = sweep(gm, (DZ, DU, DC), (dz0, dU, dth))
    parts = []
    for use in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        tans = (dz0 if use[0] else None, dU if use[1] else None, dth if use[2] else None)
        ref = TC.tangent_recursion(DZ, DU, DC, *tans); abs_ = TC.tangent_magnitudes(DZ, DU, DC, *tans)
        outs = []
        for fill in (None, np.nan):
            unread = lambda a: None if fill is None else np.full_like(a, np.nan)
            rec = (DZ, DU if use[1] else unread(DU), DC if use[2] else unread(DC))
            outs.append(sweep(gm, rec, tans))
            TC.check(outs[-1], ref, abs_, H, TC.n_terms(DZ, tans[1], tans[2]), dtype == "f32", what="inputs %s, unread Jacobians %s" % (use, "NULL" if fill is None else "NaN"))
        assert np.array_equal(outs[0], outs[1])
        if sum(use) == 1:
            parts.append(ref)
    # the three inputs act linearly: the references of the single inputs add up to the reference of all three (a check of the cases, not of the kernel)
    ref_full = TC.tangent_recursion(DZ, DU, DC, dz0, dU, dth)
    assert np.allclose(sum(parts), ref_full, rtol=1e-9, atol=1e-9) and np.isfinite(full).all()


@pytest.mark.parametrize("name", ["fixed3", "cartpole"])
def test_inputs_without_columns_are_ignored(name):
    """nu = 0: dU is ignored (fixed3); Nc = 0: dtheta is ignored (cartpole) -- whatever they point to; alone, they are no input at all"""
    H, B, T = 2, 3, 4
    gm = O._handle(name, "f64", B); nx, nu = gm.spec.nx, gm.spec.nu
    rec = TC.record(name, "f64", H, B)
    dz0, dU, _ = TC.tangents("f64", H, B, T, nx, nu, 0)
    junk = dev(np.full(64, np.nan))
    base = sweep(gm, rec, (dz0, dU, None), raw=True)
    out = guarded((H, B, T, nx), torch.float64)
    keep = [dev(a) for a in (rec[0], rec[1], dz0, dU)]
    if name == "fixed3":
        assert nu == 0
        rc = tangent_raw(gm, H, T, keep[0], None, None, keep[2], junk, None, dZ=out)
    else:
        assert len(gm.spec.contacts) == 0
        rc = tangent_raw(gm, H, T, keep[0], keep[1], None, keep[2], keep[3], junk, dZ=out)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(out, base) and guards_intact(out)
    ignored = dict(dU=junk) if name == "fixed3" else dict(dth=junk)
    rc = tangent_raw(gm, H, T, keep[0], keep[1], None, None, ignored.get("dU"), ignored.get("dth"), dZ=out)
    assert rc == INVALID and "all NULL" in gm.last_error()


# ---------------------------------------------------------------- 7. argument errors ----------------------------------------------------------------
def test_argument_errors():
    """every refusal of dojo_rollout_tangent_dev: DOJO_ERR_INVALID, a text on the handle that names the entry, nothing launched (the output stays NaN)"""
    H, B, T = 2, 3, 4
    gm = D._handle("ant", "f64", B); s = gm.spec; nx, nu, nth = s.nx, s.nu, 5 * len(s.contacts)
    DZ, DU, DC = (dev(a) for a in TC.record("ant", "f64", H, B, data=True))
    dz0, dU, dth = (dev(a) for a in TC.tangents("f64", H, B, T, nx, nu, nth))
    Z = torch.zeros((H, B, s.nz), dtype=torch.float64, device="cuda")
    out = torch.full((H, B, T, s.nz), float("nan"), dtype=torch.float64, device="cuda")
    good = dict(H=H, T=T, DZ=DZ, DU=DU, DC=DC, dz0=dz0, dU=dU, dth=dth, tan_space=0, Z=Z, status=None, dZ=out)
    bad = {"H < 1": dict(H=0), "T < 1": dict(T=0), "DZ NULL": dict(DZ=None), "dZ NULL": dict(dZ=None), "all three inputs NULL": dict(dz0=None, dU=None, dth=None),
           "dU without DU": dict(DU=None), "dtheta without DC": dict(DC=None), "tan_space 1 without Z": dict(tan_space=1, Z=None), "tan_space 2": dict(tan_space=2),
           "tan_space -1": dict(tan_space=-1), "DZ unaligned": dict(DZ=DZ.view(-1)[1:]), "DU unaligned": dict(DU=DU.view(-1)[1:]), "DC unaligned": dict(DC=DC.view(-1)[1:])}
    for what, kw in bad.items():
        a = dict(good); a.update(kw)
        rc = tangent_raw(gm, **a)
        torch.cuda.synchronize()
        msg = gm.last_error()
        assert rc == INVALID, (what, rc, msg)
        assert "dojo_rollout_tangent_dev: " in msg and len(msg) > len("dojo_rollout_tangent_dev: "), (what, msg)
        if "unaligned" in what:
            assert "16-byte" in msg, msg
        assert torch.isnan(out).all(), what
    # an unaligned Jacobian array that is not read is not refused; neither is an aligned offset into a buffer
    a = dict(good, dU=None, DU=DU.view(-1)[1:])
    assert tangent_raw(gm, **a) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out.view(-1)[:H * B * T * nx]).all()


# ---------------------------------------------------------------- 8. real rollouts ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole", "pendulum"])
def test_tangents_are_the_derivative_of_the_rollout(name):
    """(a) on the inputs of O.fd_chain_error (B 8, H 6, rtol = btol = 1e-9, GRAD_CONSISTENT, U = 0, the same seeds for W and D): sum W . dZ_state from
    rollout_tangents(dU = D, tan_space = "state") against the same central differences, under the existing test's conditions; and against the adjoint's
    <gU, D>, which is the same number to rounding"""
    B, H, ndir, eps = 8, 6, 4, 1e-6
    spec = O._spec(name)
    gm = api.BatchedMechanism(spec, B, dtype="f64", opts=d.SolverOptions(rtol=1e-9, btol=1e-9))
    try:
        gm.set_gradient_mode(api.GRAD_CONSISTENT)
        z0, _ = d.synthetic_inputs(spec, B)
        rng = np.random.default_rng(21)
        W = rng.standard_normal((H, B, spec.Nb, 13)); W[..., 6:10] = 0.0; W = W.reshape(H, B, spec.nz)
        U0 = np.zeros((H, B, spec.nu))
        _, st0, gU, _ = gm.rollout_gradients(z0, U0, W, cot_space="state")
        Ds = [rng.standard_normal(U0.shape) for _ in range(ndir)]
        dU = np.ascontiguousarray(np.stack(Ds, axis=2))                  # [H,B,T,nu]
        Zt, stt, dZ = gm.rollout_tangents(z0, U0, dU=dU, tan_space="state")
        assert np.array_equal(stt, st0)
        fwd = np.einsum("kbi,kbti->bt", W, dZ)
        rev = np.einsum("kbc,kbtc->bt", gU, dU)
        # the rounding bound of fwd = rev: the magnitudes over the record of the same rollout
        rc, Zr, sr, DZ, DU = O.record(gm, z0, U0, H)
        assert rc == 0 and np.array_equal(Zr, Zt)
        Wt = np.abs(W.reshape(H, B, spec.Nb, 13)[..., [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12]]); Wt[..., 6:9] = 0.0       # W pulled back: x, v, omega copied, no quaternion part
        s = np.einsum("kbr,kbtr->bt", Wt.reshape(H, B, spec.nx), TC.tangent_magnitudes(DZ, DU, None, None, dU, None, sr))
        lim = TC.identity_limit(H, spec.nx, spec.nu, 0, s, s)
        print("%s: largest |<W, dZ> - <gU, D>| / rounding bound = %.3f" % (name, S.ratio(fwd, rev, lim)))
        assert (np.abs(fwd - rev) <= lim).all()
        worst, counted = 0.0, np.ones(B, bool)
        for t, Dd in enumerate(Ds):
            Zp, sp = gm.rollout(z0, U0 + eps * Dd); Zm, sm = gm.rollout(z0, U0 - eps * Dd)
            ok = (st0 == 0).all(0) & (sp == 0).all(0) & (sm == 0).all(0)
            counted &= ok
            fd = ((W * (Zp - Zm)).sum(axis=(0, 2)) / (2 * eps))[ok]
            an = fwd[ok, t]
            if ok.any():
                worst = max(worst, float((np.abs(fd - an) / np.maximum(1.0, np.abs(an))).max()))
        print("%s: worst |fd - an| / max(1, |an|) = %.3e over %.0f %% of the environments" % (name, worst, 100 * counted.mean()))
        assert counted.mean() >= 0.9
        assert worst <= 1e-5
    finally:
        gm.close()


def example():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))
    import sphere_system_identification_device as ex
    return ex


def test_sphere_sensitivities_are_the_forward_chain_over_the_record():
    """(b) sphere, B 10, H 3, on the reference dataset rows the example uses: dZ for dtheta = I_5 against the NumPy forward chain dc = DC_k + DZ_k dc over the
    record's own DZ, DC (dojo_rollout_data_record_dev on torch tensors)"""
    ex = example()
    Zd = ex.dataset(); B, H = len(Zd), len(ex.TIMESTEPS)
    z0 = Zd[:, ex.TIMESTEPS[0] - 1].copy()
    gm = api.BatchedMechanism(ex.sphere(np.array([0.12, 0.47])), B, dtype="f64")
    try:
        rc, Zr, sr, DZ, DU, DC = D.record(gm, z0, None, H)
        assert rc == 0 and (sr == 0).all()
        Zt, stt, dZ = gm.rollout_tangents(z0, dtheta=np.eye(5), steps=H)
        assert np.array_equal(Zt, Zr) and np.array_equal(stt, sr) and dZ.shape == (H, B, 5, 12)
        dc = np.zeros((B, 12, 5)); ac = np.zeros((B, 12, 5))
        for k in range(H):
            Az, Ac = DZ[k].transpose(0, 2, 1), DC[k].transpose(0, 2, 1)  # the device's [B,c,r] -> [B,r,c]
            dc = Ac + Az @ dc; ac = np.abs(Ac) + np.abs(Az) @ ac
            TC.check(dZ[k].transpose(0, 2, 1), dc, ac, k + 1, 12 + 5, False, what="step %d" % k)
        assert np.abs(dc).max() > 1e-3
    finally:
        gm.close()


# ---------------------------------------------------------------- 9. end to end ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_host_entry_is_record_plus_sweep(dtype):
    """dojo_rollout_tangents (host pointers) = dojo_rollout_record_dev + dojo_rollout_tangent_dev, bit for bit, in both output spaces"""
    H, B, T = 2, 3, 5
    spec = O._spec("cartpole")
    gm = O._handle("cartpole", dtype, B); nx, nu = spec.nx, spec.nu
    z0, u = d.synthetic_inputs(spec, B)
    U = np.stack([u * f for f in (0.9, 0.6)]).astype(gm.np_dtype); z0 = z0.astype(gm.np_dtype)
    dz0, dU, _ = TC.tangents(dtype, H, B, T, nx, nu, 0)
    rc, Zr, sr, DZ, DU = O.record(gm, z0, U, H)
    assert rc == 0 and (sr == 0).all()
    for space in ("tangent", "state"):
        Zh, sh, dZh = gm.rollout_tangents(z0, U, dz0=dz0, dU=dU, tan_space=space)
        assert np.array_equal(Zh, Zr) and np.array_equal(sh, sr)
        dev = sweep(gm, (DZ, DU, None), (dz0, dU, None), tan_space=1 if space == "state" else 0, Z=Zr, status=sr)
        assert np.array_equal(dZh, dev) and np.abs(dev).max() > 0
    # dU alone, no U: the controls are zeros, DZ and DU are recorded
    Zh, sh, dZh = gm.rollout_tangents(z0, dU=dU)
    assert dZh.shape == (H, B, T, nx) and np.isfinite(dZh).all()
    with pytest.raises(ValueError):
        gm.rollout_tangents(z0, U, dz0=dz0[:, :3], dU=dU)                 # T = 3 against T = 5


def test_call_larger_than_the_device_is_refused():
    """a horizon whose record is at least twice the device's memory: DOJO_ERR_INVALID before anything is read, allocated or launched (the host arrays are
    one-element dummies), with the entry's name, the record's exact byte count and the free device memory in the text; the handle then works"""
    B, w, T = 3, 8, 2
    spec = d.get_mechanism("sphere"); nx, nu, nth = spec.nx, spec.nu, 5 * len(spec.contacts)
    per_step = B * nx * (nx + nu + nth) * w
    total = torch.cuda.mem_get_info()[1]
    H = -(-2 * total // per_step)
    record = H * per_step
    assert record >= 2 * total and H < 2 ** 31 and record * T < 2 ** 55
    gm = api.BatchedMechanism(spec, B, dtype="f64")
    try:
        one, out = np.zeros(1), np.full(1, 77.0)
        p = api.addr
        rc = api.lib().dojo_rollout_tangents(gm.h, p(one), None, H, T, p(one), p(one), p(one), 0, None, None, p(out))
        err = gm.last_error()
        print("H", H, "record", record, "rc", rc, err)
        assert rc == INVALID and "dojo_rollout_tangents" in err and str(record) in err and "free device memory" in err, (rc, err)
        assert out[0] == 77.0
        # without dU and dtheta the record is DZ alone
        rc = api.lib().dojo_rollout_tangents(gm.h, p(one), None, H, T, p(one), None, None, 0, None, None, p(out))
        assert rc == INVALID and str(H * B * nx * nx * w) in gm.last_error()
        z0 = D.floor_states(spec, B)[0]
        Z, st, dZ = gm.rollout_tangents(z0, dtheta=np.eye(5), steps=2)
        assert np.isfinite(dZ).all() and (dZ[st != 0] == 0).all() and np.abs(dZ[st == 0]).max() > 0      # (these states make some first steps fail: zeros there)
    finally:
        gm.close()


# ---------------------------------------------------------------- 10. the example ----------------------------------------------------------------
def test_gauss_newton_example_in_forward_mode():
    """examples/sphere_system_identification_device.py --gauss-newton: (cost, g, H) of the one-handle forward-mode path against the default path's (fp64 products
    of the same three 12 x 12 Jacobians per trajectory in another summation order), and the reference's quasi-Newton loop on it recovers [0.2, 0.5]"""
    ex = example()
    Zd = ex.dataset()
    fm = ex.ForwardModeLoss(Zd)
    try:
        th5 = np.array([0.12, 0.47, 0.0, 0.0, 0.0])
        c, g, H = fm.fgH(th5)
        c0, g0, H0 = ex.loss(th5, Zd, derivatives=True)
        for what, a, b in (("cost", np.array([c]), np.array([c0])), ("g", g, g0), ("H", H, H0)):
            rel = np.abs(a - b).max() / np.abs(b).max()
            print("forward-mode %s against the default path: %.3e of the largest entry" % (what, rel))
            assert rel <= 1e-10
        assert abs(fm.cost(th5) - c) <= 1e-12 * max(1.0, c)
        f0 = lambda th: fm.cost(np.concatenate([th, np.zeros(3)]))
        fgH0 = lambda th: fm.fgH(np.concatenate([th, np.zeros(3)]))
        sol = ex.quasi_newton_solve(f0, fgH0, np.array([0.0, 1.0]), verbose=False)
        print("recovered friction_coefficient %.6f, contact_radius %.6f, cost %.3e" % (sol[0], sol[1], f0(sol)))
        assert abs(sol[0] - 0.2) < 5e-3 and abs(sol[1] - 0.5) < 5e-4 and f0(sol) < 1e-6
    finally:
        fm.close()
