"""Reverse-mode rollouts on the GPU: dojo_rollout_adjoint_dev against the recursion it implements (NumPy fp64 on the same values),
dojo_rollout_record_dev against the stepwise path, dojo_rollout_gradients end to end, the chain against finite differences of the
rollout, and the torch.autograd wrapper.

The recursion, per environment b, with g_k the cotangent w.r.t. the state after step k:
    lambda <- g_{H-1};  for k = H-1 .. 0:  failed step: gU[k] <- 0, lambda <- 0;  else gU[k] <- DU_k^T lambda, lambda <- DZ_k^T lambda;
                                           if k > 0: lambda <- lambda + g_{k-1};      gz <- lambda

Error bound of the kernel tests (elementwise): every output is a chain of at most H dot products of at most nx terms, each followed by one
addition of g, all in fp64; two summation orders of such a dot product differ by at most gamma_n sum |x_i y_i| each (Higham, Accuracy and
Stability of Numerical Algorithms, 3.1), so with `abs` the same recursion run on |DZ|, |DU|, |G|
    |out - ref| <= 2 H (nx + 2) 2^-53 abs   (+ 2^-23 |ref| for fp32 outputs: one rounding of the result, a whole ulp)
and (nx + 12) where the cotangent is first pulled back from state coordinates (the ten extra operations of the quaternion product)."""

import numpy as np
import pytest
import torch

import dojo_amd as d
from dojo_amd import api, quat
from gpu_util import dev

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -2


def _spec(name):
    if name == "fixed3":
        return d.get_npendulum(num_bodies=3, base_joint_type="Fixed", rest_joint_type="Fixed")
    if name == "ant":
        return d.baseline_config(3)
    return d.get_mechanism(name)


_handles = {}


def _handle(name, dtype, B):
    """one handle per (mechanism, dtype, batch) for the whole module: the synthetic cases only need its nx, nu"""
    key = (name, dtype, B)
    if key not in _handles:
        _handles[key] = api.BatchedMechanism(_spec(name), B, dtype=dtype)
    return _handles[key]


def teardown_module(module):
    for gm in _handles.values():
        gm.close()
    _handles.clear()


def adjoint_raw(gm, H, DZ, DU, G, cot_space=0, Z=None, status=None, gU=None, gz=None):
    """dojo_rollout_adjoint_dev on torch tensors (None = NULL) -> return code"""
    return api.lib().dojo_rollout_adjoint_dev(gm.h, int(H), api.addr(DZ), api.addr(DU), api.addr(G), int(cot_space), api.addr(Z), api.addr(status), api.addr(gU), api.addr(gz), api.torch_stream())


def adjoint(gm, DZ, DU, G, cot_space=0, Z=None, status=None, outs=None):
    """NumPy in, NumPy out: (gU [H,B,nu] or None, gz [B,nx]); the outputs start as NaN so that an entry the kernel leaves out shows.
    outs: the caller's own device tensors {"gU": .., "gz": ..} instead (a missing key = NULL, returned as None); DU = None is then passed as NULL"""
    H, B = G.shape[:2]
    nx, nu = gm.spec.nx, gm.spec.nu
    tdt = torch.float32 if gm.dtype_code else torch.float64
    if outs is None:
        gU = torch.full((H, B, nu), float("nan"), dtype=tdt, device="cuda") if nu else None
        gz = torch.full((B, nx), float("nan"), dtype=tdt, device="cuda")
    else:
        gU, gz = (outs.get("gU") if nu else None), outs.get("gz")
    keep = [dev(DZ), dev(DU) if nu else None, dev(G), dev(Z), dev(status)]
    api._chk(adjoint_raw(gm, H, keep[0], keep[1], keep[2], cot_space, keep[3], keep[4], gU, gz))
    torch.cuda.synchronize()
    return (None if gU is None else gU.cpu().numpy()), (None if gz is None else gz.cpu().numpy())


def recursion(DZ, DU, G, status=None):
    """the reference: fp64 NumPy; DZ [H,B,c,r], DU [H,B,c,r] or None, G [H,B,nx] tangent.  A failed step's Jacobians are not touched."""
    DZ = np.asarray(DZ, np.float64); G = np.asarray(G, np.float64)
    H, B, nx = G.shape
    nu = 0 if DU is None else DU.shape[2]
    gU = np.zeros((H, B, nu)); lam = G[H - 1].copy()
    for k in range(H - 1, -1, -1):
        ok = np.ones(B, bool) if status is None else (status[k] == 0)
        new = np.zeros((B, nx))
        new[ok] = np.einsum("bcr,br->bc", DZ[k][ok], lam[ok])
        if nu:
            gU[k][ok] = np.einsum("bcr,br->bc", np.asarray(DU[k][ok], np.float64), lam[ok])
        lam = new
        if k > 0:
            lam = lam + G[k - 1]
    return gU, lam


def bound(H, nx, extra, abs_, ref, f32):
    return 2.0 * H * (nx + extra) * 2.0 ** -53 * abs_ + (2.0 ** -23 * np.abs(ref) if f32 else 0.0)


def check(out, ref, abs_, H, nx, f32, extra=2, what=""):
    err = np.abs(out.astype(np.float64) - ref); lim = bound(H, nx, extra, abs_, ref, f32)
    assert np.isfinite(out).all(), what
    worst = (err - lim).max()
    assert worst <= 0.0, "%s: error exceeds the bound by %.3e (max error %.3e, max |ref| %.3e)" % (what, worst, err.max(), np.abs(ref).max())


_inputs = {}


def synthetic(name, dtype, H, B, seed=7):
    """DZ ~ 1.3 N(0,1) / sqrt(nx), DU, G ~ N(0,1), in the handle's dtype; made once per case"""
    key = (name, dtype, H, B, seed)
    if key not in _inputs:
        s = _spec(name); nx, nu = s.nx, s.nu
        rng = np.random.default_rng(seed); dt = np.float32 if dtype == "f32" else np.float64
        DZ = (1.3 * rng.standard_normal((H, B, nx, nx)) / np.sqrt(nx)).astype(dt)
        DU = rng.standard_normal((H, B, nu, nx)).astype(dt) if nu else None
        G = rng.standard_normal((H, B, nx)).astype(dt)
        _inputs[key] = (DZ, DU, G)
    return _inputs[key]


CASES = [(m, hb) for m in ("pendulum", "fixed3", "cartpole", "ant") for hb in ((1, 1), (2, 3), (7, 65))] + [("atlas", (3, 5))]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,hb", CASES)
def test_kernel_matches_the_recursion(name, hb, dtype):
    """1. synthetic Jacobians, no solver involved: nx = 12 (one body, fewer rows than a 16-lane row), 36 without controls (DU / gU NULL),
    24, 156 (pieces that end inside a row), 372 (more columns than lanes)"""
    H, B = hb
    gm = _handle(name, dtype, B); nx = gm.spec.nx
    DZ, DU, G = synthetic(name, dtype, H, B)
    gU, gz = adjoint(gm, DZ, DU, G)
    rU, rz = recursion(DZ, DU, G)
    aU, az = recursion(np.abs(DZ), None if DU is None else np.abs(DU), np.abs(G))
    check(gz, rz, az, H, nx, dtype == "f32", what="gz")
    if gm.spec.nu:
        check(gU, rU, aU, H, nx, dtype == "f32", what="gU")
    else:
        assert gU is None and DU is None


def pull_back(Gs, Z, f32):
    """state-space cotangent [H,B,13Nb] -> tangent [H,B,12Nb] with dojo_amd.quat: g_phi = (conj(q) (x) g_q)[1:]; and the sum of the
    magnitudes of the terms of every entry (what the error bound's `abs` recursion starts from)"""
    H, B, nz = Gs.shape
    g = np.asarray(Gs, np.float64).reshape(-1, 13); z = np.asarray(Z, np.float64).reshape(-1, 13)
    q = z[:, 6:10].T.copy()
    if f32:
        q = q / np.linalg.norm(q, axis=0)
    gq = g[:, 6:10].T
    gphi = quat.qmul(quat.qconj(q), gq)[1:].T
    aq, ag = np.abs(q), np.abs(gq)
    aphi = np.stack([aq[0] * ag[1 + a] + ag[0] * aq[1 + a] + aq[1 + (a + 1) % 3] * ag[1 + (a + 2) % 3] + aq[1 + (a + 2) % 3] * ag[1 + (a + 1) % 3] for a in range(3)], 1)
    t = np.concatenate([g[:, 0:6], gphi, g[:, 10:13]], 1).reshape(H, B, -1)
    ta = np.concatenate([np.abs(g[:, 0:6]), aphi, np.abs(g[:, 10:13])], 1).reshape(H, B, -1)
    return t, ta


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["cartpole", "ant"])
def test_state_space_cotangents(name, dtype):
    """2. cot_space = 1: G in state coordinates, pulled back through dq = q (x) (0, phi) at the states Z (random unit quaternions; fp32: rounded,
    and the kernel uses q / |q|)"""
    H, B = 3, 5
    gm = _handle(name, dtype, B); s = gm.spec; nx = s.nx
    DZ, DU, _ = synthetic(name, dtype, H, B)
    rng = np.random.default_rng(11); dt = gm.np_dtype
    Z = rng.standard_normal((H, B, s.Nb, 13))
    Z[..., 6:10] /= np.linalg.norm(Z[..., 6:10], axis=-1, keepdims=True)
    Z = Z.reshape(H, B, s.nz).astype(dt)
    Gs = rng.standard_normal((H, B, s.nz)).astype(dt)
    gU, gz = adjoint(gm, DZ, DU, Gs, cot_space=1, Z=Z)
    Gt, Ga = pull_back(Gs, Z, dtype == "f32")
    rU, rz = recursion(DZ, DU, Gt)
    aU, az = recursion(np.abs(DZ), np.abs(DU), Ga)
    check(gz, rz, az, H, nx, dtype == "f32", extra=12, what="gz")
    check(gU, rU, aU, H, nx, dtype == "f32", extra=12, what="gU")


def test_nothing_flows_through_a_failed_step():
    """3. status[2,1] = 1 and NaN Jacobians there: every output finite, environment 1 is the recursion with the cut, the others do not notice"""
    H, B = 5, 4
    gm = _handle("ant", "f64", B); nx = gm.spec.nx
    DZ, DU, G = synthetic("ant", "f64", H, B, seed=3)
    clean_U, clean_z = adjoint(gm, DZ, DU, G)
    DZn, DUn = DZ.copy(), DU.copy(); DZn[2, 1] = np.nan; DUn[2, 1] = np.nan
    status = np.zeros((H, B), np.int32); status[2, 1] = 1
    gU, gz = adjoint(gm, DZn, DUn, G, status=status)
    assert np.isfinite(gU).all() and np.isfinite(gz).all()
    rU, rz = recursion(DZn, DUn, G, status)
    DZa, DUa = np.abs(DZ), np.abs(DU)
    aU, az = recursion(DZa, DUa, np.abs(G), status)
    check(gz, rz, az, H, nx, False, what="gz"); check(gU, rU, aU, H, nx, False, what="gU")
    assert (gU[2, 1] == 0.0).all()
    for b in (0, 2, 3):
        assert np.array_equal(gU[:, b], clean_U[:, b]) and np.array_equal(gz[b], clean_z[b])
    # ... and with status all zero the result is the one without a status buffer
    zU, zz = adjoint(gm, DZ, DU, G, status=np.zeros((H, B), np.int32))
    assert np.array_equal(zU, clean_U) and np.array_equal(zz, clean_z)


def test_deterministic_and_independent_of_the_batch():
    """4. fixed summation order: two runs agree bit for bit, and so does an environment run alone (B = 1) with its place in a batch of 65"""
    H, B = 7, 65
    DZ, DU, G = synthetic("ant", "f64", H, B)
    gm = _handle("ant", "f64", B)
    gU, gz = adjoint(gm, DZ, DU, G)
    gU2, gz2 = adjoint(gm, DZ, DU, G)
    assert np.array_equal(gU, gU2) and np.array_equal(gz, gz2)
    g1 = _handle("ant", "f64", 1)
    for b in (0, 32, 64):
        sU, sz = adjoint(g1, DZ[:, b:b + 1], DU[:, b:b + 1], G[:, b:b + 1])
        assert np.array_equal(sU[:, 0], gU[:, b]) and np.array_equal(sz[0], gz[b]), b


def record(gm, z0, U, H):
    """dojo_rollout_record_dev on torch tensors -> (rc, Z, status, DZ [H,B,c,r], DU [H,B,c,r])"""
    s, B = gm.spec, gm.batch
    tdt = torch.float32 if gm.dtype_code else torch.float64
    Z = torch.empty((H, B, s.nz), dtype=tdt, device="cuda"); st = torch.empty((H, B), dtype=torch.int32, device="cuda")
    DZ = torch.empty((H, B, s.nx, s.nx), dtype=tdt, device="cuda"); DU = torch.empty((H, B, max(s.nu, 1), s.nx), dtype=tdt, device="cuda")
    z0d, Ud = dev(z0.astype(gm.np_dtype)), dev(None if U is None else U.astype(gm.np_dtype))
    rc = api.lib().dojo_rollout_record_dev(gm.h, api.addr(z0d), api.addr(Ud), int(H), api.addr(Z), api.addr(st), api.addr(DZ), api.addr(DU), api.torch_stream())
    torch.cuda.synchronize()
    return rc, Z.cpu().numpy(), st.cpu().numpy(), DZ.cpu().numpy(), DU.cpu().numpy()[:, :, :s.nu]


_stepwise = {}


def ant_stepwise(B, H):
    """Ant f64 through the EXISTING paths, once per shape: rollout, and step(with_gradient) + gradients() from the rollout's states"""
    if (B, H) not in _stepwise:
        spec = _spec("ant")
        z0, u = d.synthetic_inputs(spec, B)
        rng = np.random.default_rng(5)
        U = np.stack([u * rng.uniform(0.5, 1.0) for _ in range(H)])
        gm = _handle("ant", "f64", B)
        Z, st = gm.rollout(z0, U)
        DZ, DU = [], []
        for k in range(H):
            zn, sk, _ = gm.step(z0 if k == 0 else Z[k - 1], U[k], with_gradient=True)
            assert np.array_equal(zn, Z[k]) and np.array_equal(sk, st[k])
            dz, du = gm.gradients()
            DZ.append(dz.transpose(0, 2, 1)); DU.append(du.transpose(0, 2, 1))      # row-major [B,r,c] -> the device's [B,c,r]
        _stepwise[(B, H)] = (z0, U, Z, st, np.stack(DZ), np.stack(DU))
    return _stepwise[(B, H)]


@pytest.mark.parametrize("B,H", [(64, 4), (600, 3)])
def test_record_is_the_stepwise_path(B, H):
    """5. dojo_rollout_record_dev: states and status of dojo_rollout, Jacobians of dojo_step + dojo_gradients, bit for bit (600 environments:
    several environment groups)"""
    z0, U, Z, st, DZ, DU = ant_stepwise(B, H)
    rc, Zr, sr, DZr, DUr = record(_handle("ant", "f64", B), z0, U, H)
    assert rc == 0
    assert np.array_equal(Zr, Z) and np.array_equal(sr, st)
    ok = sr == 0                                                             # (what a failed step leaves in its Jacobians is nobody's contract)
    assert ok.mean() > 0.9
    assert np.isfinite(DZr[ok]).all() and np.isfinite(DUr[ok]).all()
    assert np.array_equal(DZr[ok], DZ[ok]) and np.array_equal(DUr[ok], DU[ok])


def test_record_refuses_mechanisms_without_gradients():
    spec = d.get_mechanism("sphere", contact_type="linear")
    gm = api.BatchedMechanism(spec, 4, dtype="f64")
    try:
        z0 = np.tile(d.initialize(spec), (4, 1))
        rc, _, _, _, _ = record(gm, z0, None, 2)
        assert rc == UNSUPPORTED and "LinearContact" in gm.last_error()
    finally:
        gm.close()


def test_rollout_gradients_end_to_end():
    """6. the host entry on real Jacobians: against the recursion over the Jacobians of the existing step / gradients path, cut at the
    device's own status"""
    B, H = 64, 4
    z0, U, Z, st, DZ, DU = ant_stepwise(B, H)
    gm = _handle("ant", "f64", B); nx = gm.spec.nx
    G = np.random.default_rng(9).standard_normal((H, B, nx))
    Zg, sg, gU, gz = gm.rollout_gradients(z0, U, G)
    assert np.array_equal(Zg, Z) and np.array_equal(sg, st)
    rU, rz = recursion(DZ, DU, G, st)
    aU, az = recursion(np.abs(DZ), np.abs(DU), np.abs(G), st)
    check(gz, rz, az, H, nx, False, what="gz"); check(gU, rU, aU, H, nx, False, what="gU")
    assert np.abs(rU).max() > 0


def fd_chain_error(name, B=8, H=6, ndir=4, eps=1e-6):
    """-> (worst |fd - an| / max(1, |an|) over the counted environments and directions, fraction of environments counted): the adjoint's
    <gU, D> against central differences of the existing rollout, loss linear in the x, v, omega components of every state"""
    spec = _spec(name)
    gm = api.BatchedMechanism(spec, B, dtype="f64", opts=d.SolverOptions(rtol=1e-9, btol=1e-9))
    try:
        gm.set_gradient_mode(api.GRAD_CONSISTENT)
        z0, _ = d.synthetic_inputs(spec, B)
        rng = np.random.default_rng(21)
        W = rng.standard_normal((H, B, spec.Nb, 13)); W[..., 6:10] = 0.0; W = W.reshape(H, B, spec.nz)
        U0 = np.zeros((H, B, spec.nu))
        _, st0, gU, _ = gm.rollout_gradients(z0, U0, W, cot_space="state")
        worst, counted = 0.0, np.ones(B, bool)
        for _ in range(ndir):
            D = rng.standard_normal(U0.shape)
            Zp, sp = gm.rollout(z0, U0 + eps * D); Zm, sm = gm.rollout(z0, U0 - eps * D)
            ok = (st0 == 0).all(0) & (sp == 0).all(0) & (sm == 0).all(0)
            counted &= ok
            fd = ((W * (Zp - Zm)).sum(axis=(0, 2)) / (2 * eps))[ok]
            an = (gU * D).sum(axis=(0, 2))[ok]
            if ok.any():
                worst = max(worst, float((np.abs(fd - an) / np.maximum(1.0, np.abs(an))).max()))
        return worst, counted.mean()
    finally:
        gm.close()


@pytest.mark.parametrize("name", ["cartpole", "pendulum"])
def test_chain_is_the_derivative_of_the_rollout(name):
    """7. GRAD_CONSISTENT, rtol = btol = 1e-9, U = 0, H = 6: the chain against central differences (eps 1e-6) along 4 random directions"""
    worst, frac = fd_chain_error(name)
    print("%s: worst |fd - an| / max(1, |an|) = %.3e over %.0f %% of the environments" % (name, worst, 100 * frac))
    assert frac >= 0.9
    assert worst <= 1e-5
    if name == "cartpole":
        w_ant, f_ant = fd_chain_error("ant")
        print("ant (contacts, not asserted): worst %.3e over %.0f %% of the environments" % (w_ant, 100 * f_ant))


def lift(gz, z0, f32):
    """[B,nx] tangent -> [B,13Nb] state at z0 with dojo_amd.quat: g_q = q0 (x) (0, g_phi)"""
    B = gz.shape[0]
    g = np.asarray(gz, np.float64).reshape(-1, 12); z = np.asarray(z0, np.float64).reshape(-1, 13)
    q = z[:, 6:10].T.copy()
    if f32:
        q = q / np.linalg.norm(q, axis=0)
    gq = quat.qmul(q, np.concatenate([np.zeros((1, g.shape[0])), g[:, 6:9].T])).T
    return np.concatenate([g[:, 0:6], gq, g[:, 9:12]], 1).reshape(B, -1)


def test_autograd_wrapper():
    """8. torch.autograd through differentiable_rollout: the U gradient is the host entry's gU bit for bit (same kernels, same buffers' contents),
    the z0 gradient its gz lifted to state shape (formed in fp64 by both sides -- torch on the device, NumPy here -- and rounded once to fp32: equal to
    within one unit in the last place of each entry)"""
    from dojo_amd.autograd import differentiable_rollout
    B, H = 16, 5
    spec = _spec("cartpole")
    gm = _handle("cartpole", "f32", B)
    z0, u = d.synthetic_inputs(spec, B)
    rng = np.random.default_rng(13)
    U = np.stack([u * rng.uniform(0.5, 1.0) for _ in range(H)]).astype(np.float32); z0 = z0.astype(np.float32)
    W = rng.standard_normal((H, B, spec.nz)).astype(np.float32)
    Zh, sh, gU, gz = gm.rollout_gradients(z0, U, W, cot_space="state")
    zt = dev(z0).requires_grad_(True); Ut = dev(U).requires_grad_(True)
    Z = differentiable_rollout(gm, zt, Ut)
    assert Z.status.dtype == torch.int32 and not Z.status.requires_grad
    gzt, gUt = torch.autograd.grad((Z * dev(W)).sum(), [zt, Ut])
    torch.cuda.synchronize()
    assert np.array_equal(Z.detach().cpu().numpy(), Zh) and np.array_equal(Z.status.cpu().numpy(), sh)
    assert np.array_equal(gUt.cpu().numpy(), gU) and np.abs(gU).max() > 0
    ref = lift(gz, z0, True).astype(np.float32)                              # rounded once, like the wrapper's
    got = gzt.cpu().numpy()
    assert got.dtype == np.float32 and np.abs(ref).max() > 0
    assert np.all(np.abs(got - ref) <= np.spacing(np.abs(ref)))                # one unit in the last place of every entry, nothing absolute


def test_argument_errors():
    """9. every argument error of dojo_rollout_adjoint_dev: DOJO_ERR_INVALID, a message on the handle, nothing launched (the outputs keep their fill)"""
    H, B = 2, 3
    gm = _handle("cartpole", "f64", B); s = gm.spec
    DZ, DU, G = (dev(a) for a in synthetic("cartpole", "f64", H, B))
    Z = torch.zeros((H, B, s.nz), dtype=torch.float64, device="cuda")
    gU = torch.full((H, B, s.nu), 77.0, dtype=torch.float64, device="cuda"); gz = torch.full((B, s.nx), 77.0, dtype=torch.float64, device="cuda")
    bad = {"H < 1": dict(H=0), "DZ NULL": dict(DZ=None), "G NULL": dict(G=None), "cot_space 1 without Z": dict(cot_space=1, Z=None),
           "gU without DU": dict(DU=None)}
    for what, kw in bad.items():
        a = dict(H=H, DZ=DZ, DU=DU, G=G, cot_space=0, Z=Z, status=None, gU=gU, gz=gz); a.update(kw)
        rc = adjoint_raw(gm, a.pop("H"), a.pop("DZ"), a.pop("DU"), a.pop("G"), **a)
        torch.cuda.synchronize()
        assert rc == INVALID, what
        msg = gm.last_error()
        assert "dojo_rollout_adjoint_dev" in msg, (what, msg)
        assert (gU == 77.0).all() and (gz == 77.0).all(), what
    # the kernel reads DZ and DU in 16-byte pieces: a pointer into the middle of a piece is refused (an aligned offset into a buffer is fine)
    for what, kw in {"DZ unaligned": dict(DZ=DZ.view(-1)[1:]), "DU unaligned": dict(DU=DU.view(-1)[1:])}.items():
        a = dict(H=1, DZ=DZ, DU=DU, G=G, cot_space=0, Z=Z, status=None, gU=gU, gz=gz); a.update(kw)
        rc = adjoint_raw(gm, a.pop("H"), a.pop("DZ"), a.pop("DU"), a.pop("G"), **a)
        torch.cuda.synchronize()
        assert rc == INVALID and "16-byte" in gm.last_error(), (what, gm.last_error())
        assert (gU == 77.0).all() and (gz == 77.0).all(), what
    # DU may be NULL when no gU is asked for
    assert adjoint_raw(gm, H, DZ, None, G, 0, None, None, None, gz) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(gz).all() and not (gz == 77.0).all()
