"""Contact-data gradients through rollouts on the GPU: dojo_rollout_data_adjoint_dev against the recursion it implements (NumPy fp64 on the same
values), dojo_rollout_data_record_dev against the stepwise path, dojo_set_contact_data against a fresh handle, dojo_rollout_data_gradients end to
end, the chain against finite differences of the rollout in theta, and the torch.autograd wrapper.

The recursion, per environment b, with g_k the cotangent w.r.t. the state after step k and theta = [friction, radius, origin(3)] per contact:
    lambda <- g_{H-1}; a <- 0;  for k = H-1 .. 0:  failed step: lambda <- 0;  else a <- a + DC_k^T lambda, lambda <- DZ_k^T lambda;
                                                   if k > 0: lambda <- lambda + g_{k-1};      gtheta_env <- a;  gz <- lambda;  gtheta <- sum_b a_b

Error bound of the kernel tests (elementwise), derived as in tests/test_rollout_adjoint_gpu.py: every output is a chain of at most H dot products of
at most nx terms, all in fp64.  For gz each is followed by one addition (of g); an entry of a is a dot product with lambda_k = (what step k + 1 left)
+ g_k -- that addition -- followed by the addition into the accumulator: one more per step than gU has.  Two summation orders of a dot product of n
terms differ by at most gamma_n sum |x_i y_i| each (Higham, Accuracy and Stability of Numerical Algorithms, 3.1), so with `abs` the same recursion
run on |DZ|, |DC|, |G|
    |out - ref| <= 2 H (nx + 3) 2^-53 abs   (+ 2^-23 |ref| for fp32 outputs: one rounding of the result, a whole ulp)
and (nx + 13) where the cotangent is first pulled back from state coordinates (the ten extra operations of the quaternion product).
The shared sum: gtheta = sum_b a_b is formed by the device in a fixed tree (256 lanes add every 256th environment in ascending order, then two levels of
four DPP stages; a stage that adds a zero does not round), of depth ceil(log2 B) for B <= 256 -- inside the ceil(log2 B) + 1 roundings counted here; the
reference adds the a_b in extended precision.  Each of those roundings is relative to a partial sum bounded by
sum_b abs_b, on top of the errors the a_b carry:
    |gtheta - ref| <= sum_b 2 H (nx + 3) 2^-53 abs_b + (ceil(log2 B) + 1) 2^-53 sum_b abs_b   (+ 2^-23 |ref| for fp32 outputs)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dojo_amd as d
from dojo_amd import api, quat
from gpu_util import dev, same

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -2


def _spec(name):
    if name == "ant":
        return d.baseline_config(3)
    if name == "block":
        return d.get_mechanism("block", contact_corners=4)
    if name == "sliding_sphere":
        return d.get_mechanism("sphere", friction_coefficient=0.2)
    return d.get_mechanism(name)


def floor_states(spec, B, seed=29):
    """a one-body mechanism (sphere, block) resting on the floor, upright, with a horizontal velocity, a small downward one and a spin per environment:
    the contacts are active from the first step on, so that the contact data matter; and controls N(0, 0.5) for the floating base"""
    rng = np.random.default_rng(seed)
    z = np.tile(d.initialize(spec, position=[0.0, 0.0, 0.0]), (B, 1))
    z[:, 3:5] = rng.uniform(-1.0, 1.0, (B, 2)); z[:, 5] = -0.1; z[:, 10:13] = 0.5 * rng.standard_normal((B, 3))
    return z, 0.5 * rng.standard_normal((B, spec.nu))


_handles = {}


def _handle(name, dtype, B):
    """one handle per (mechanism, dtype, batch) for the whole module: the synthetic cases only need its nx, Nc"""
    key = (name, dtype, B)
    if key not in _handles:
        _handles[key] = api.BatchedMechanism(_spec(name), B, dtype=dtype)
    return _handles[key]


def teardown_module(module):
    for gm in _handles.values():
        gm.close()
    _handles.clear()


def _nth(gm):
    return 5 * len(gm.spec.contacts)


def data_adjoint_raw(gm, H, DZ, DC, G, cot_space=0, Z=None, status=None, gte=None, gt=None, gz=None):
    """dojo_rollout_data_adjoint_dev on torch tensors (None = NULL) -> return code"""
    return api.lib().dojo_rollout_data_adjoint_dev(gm.h, int(H), api.addr(DZ), api.addr(DC), api.addr(G), int(cot_space), api.addr(Z), api.addr(status), api.addr(gte), api.addr(gt), api.addr(gz), api.torch_stream())


def data_adjoint(gm, DZ, DC, G, cot_space=0, Z=None, status=None, want=("env", "sum", "gz"), outs=None):
    """NumPy in, NumPy out: (gtheta_env [B,nth], gtheta [nth], gz [B,nx]), None where not asked for; the outputs start as NaN so that an entry
    the kernels leave out shows.  outs: the caller's own device tensors {"env": .., "sum": .., "gz": ..} for the outputs in `want` instead"""
    H, B = G.shape[:2]
    nx, nth = gm.spec.nx, _nth(gm)
    tdt = torch.float32 if gm.dtype_code else torch.float64
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=tdt, device="cuda")
    own = lambda k, *shape: None if k not in want else nan(*shape) if outs is None else outs[k]
    gte, gt, gz = own("env", B, nth), own("sum", nth), own("gz", B, nx)
    keep = [dev(DZ), dev(DC), dev(G), dev(Z), dev(status)]
    api._chk(data_adjoint_raw(gm, H, keep[0], keep[1], keep[2], cot_space, keep[3], keep[4], gte, gt, gz))
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (gte, gt, gz))


def recursion(DZ, DC, G, status=None):
    """the reference: fp64 NumPy; DZ [H,B,c,r], DC [H,B,c,r], G [H,B,nx] tangent -> (a [B,nth], lambda [B,nx]).  A failed step's Jacobians are
    not touched."""
    DZ = np.asarray(DZ, np.float64); DC = np.asarray(DC, np.float64); G = np.asarray(G, np.float64)
    H, B, nx = G.shape
    a = np.zeros((B, DC.shape[2])); lam = G[H - 1].copy()
    for k in range(H - 1, -1, -1):
        ok = np.ones(B, bool) if status is None else (status[k] == 0)
        new = np.zeros((B, nx))
        new[ok] = np.einsum("bcr,br->bc", DZ[k][ok], lam[ok])
        a[ok] += np.einsum("bcr,br->bc", DC[k][ok], lam[ok])
        lam = new
        if k > 0:
            lam = lam + G[k - 1]
    return a, lam


def bound(H, nx, extra, abs_, ref, f32):
    return 2.0 * H * (nx + extra) * 2.0 ** -53 * abs_ + (2.0 ** -23 * np.abs(ref) if f32 else 0.0)


def check(out, ref, abs_, H, nx, f32, extra=3, what=""):
    err = np.abs(out.astype(np.float64) - ref); lim = bound(H, nx, extra, abs_, ref, f32)
    assert np.isfinite(out).all(), what
    worst = (err - lim).max()
    print("%s: max error %.3e, smallest margin to the bound %.3e" % (what, err.max(), -worst))
    assert worst <= 0.0, "%s: error exceeds the bound by %.3e (max error %.3e, max |ref| %.3e)" % (what, worst, err.max(), np.abs(ref).max())


def batch_sum(a):
    """sum over the batch in extended precision (the reference of the shared sum carries no rounding of its own worth counting)"""
    return np.asarray(np.asarray(a, np.longdouble).sum(0), np.float64)


def check_sum(out, ra, aa, H, nx, f32, extra=3, what="gtheta"):
    """the shared sum against sum_b of the per-environment reference, with the bound of the module docstring"""
    B = ra.shape[0]
    ref = batch_sum(ra); asum = batch_sum(aa)
    lim = 2.0 * H * (nx + extra) * 2.0 ** -53 * asum + (math.ceil(math.log2(B)) + 1) * 2.0 ** -53 * asum + (2.0 ** -23 * np.abs(ref) if f32 else 0.0)
    err = np.abs(out.astype(np.float64) - ref)
    assert np.isfinite(out).all(), what
    worst = (err - lim).max()
    print("%s: max error %.3e, smallest margin to the bound %.3e" % (what, err.max(), -worst))
    assert worst <= 0.0, "%s: error exceeds the bound by %.3e (max error %.3e, max |ref| %.3e)" % (what, worst, err.max(), np.abs(ref).max())


_inputs = {}


def synthetic(name, dtype, H, B, seed=7):
    """DZ ~ 1.3 N(0,1) / sqrt(nx), DC, G ~ N(0,1), in the handle's dtype; made once per case"""
    key = (name, dtype, H, B, seed)
    if key not in _inputs:
        s = _spec(name); nx, nth = s.nx, 5 * len(s.contacts)
        rng = np.random.default_rng(seed); dt = np.float32 if dtype == "f32" else np.float64
        DZ = (1.3 * rng.standard_normal((H, B, nx, nx)) / np.sqrt(nx)).astype(dt)
        DC = rng.standard_normal((H, B, nth, nx)).astype(dt)
        G = rng.standard_normal((H, B, nx)).astype(dt)
        _inputs[key] = (DZ, DC, G)
    return _inputs[key]


CASES = [(m, hb) for m in ("sphere", "block", "ant") for hb in ((1, 1), (2, 3), (7, 65))] + [("atlas", (3, 5))]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,hb", CASES)
def test_kernel_matches_the_recursion(name, hb, dtype):
    """1. synthetic Jacobians, no solver involved: sphere (nx 12, 5 contact-data columns: fewer than one column group of 64), block with four corners
    (20 columns), ant (nx 156: pieces that end inside a row, 20 columns), atlas (more rows than lanes, 100 columns).  Three calls: gtheta_env and gz; gz = NULL, so
    that step 0 starts at column nx and the columns of DC sit on other lanes than in the steps before; gtheta alone (the workspace and the reduction)."""
    H, B = hb
    gm = _handle(name, dtype, B); nx = gm.spec.nx; f32 = dtype == "f32"
    assert _nth(gm) > 0
    DZ, DC, G = synthetic(name, dtype, H, B)
    ra, rz = recursion(DZ, DC, G)
    aa, az = recursion(np.abs(DZ), np.abs(DC), np.abs(G))
    gte, gt, gz = data_adjoint(gm, DZ, DC, G, want=("env", "gz"))
    assert gt is None
    check(gz, rz, az, H, nx, f32, what="gz"); check(gte, ra, aa, H, nx, f32, what="gtheta_env")
    gte0, _, gz0 = data_adjoint(gm, DZ, DC, G, want=("env",))
    assert gz0 is None
    check(gte0, ra, aa, H, nx, f32, what="gtheta_env without gz")
    _, gt, _ = data_adjoint(gm, DZ, DC, G, want=("sum",))
    check_sum(gt, ra, aa, H, nx, f32)


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
def test_state_space_cotangents(dtype):
    """2. cot_space = 1: G in state coordinates, pulled back through dq = q (x) (0, phi) at the states Z (random unit quaternions; fp32: rounded,
    and the kernel uses q / |q|)"""
    H, B = 3, 5
    gm = _handle("ant", dtype, B); s = gm.spec; nx = s.nx; f32 = dtype == "f32"
    DZ, DC, _ = synthetic("ant", dtype, H, B)
    rng = np.random.default_rng(11); dt = gm.np_dtype
    Z = rng.standard_normal((H, B, s.Nb, 13))
    Z[..., 6:10] /= np.linalg.norm(Z[..., 6:10], axis=-1, keepdims=True)
    Z = Z.reshape(H, B, s.nz).astype(dt)
    Gs = rng.standard_normal((H, B, s.nz)).astype(dt)
    gte, gt, gz = data_adjoint(gm, DZ, DC, Gs, cot_space=1, Z=Z)
    Gt, Ga = pull_back(Gs, Z, f32)
    ra, rz = recursion(DZ, DC, Gt)
    aa, az = recursion(np.abs(DZ), np.abs(DC), Ga)
    check(gz, rz, az, H, nx, f32, extra=13, what="gz")
    check(gte, ra, aa, H, nx, f32, extra=13, what="gtheta_env")
    check_sum(gt, ra, aa, H, nx, f32, extra=13)


def test_nothing_flows_through_a_failed_step():
    """3. status[2,1] = 1 and NaN Jacobians there: every output finite, environment 1 is the recursion with the cut, the others do not notice"""
    H, B = 5, 4
    gm = _handle("ant", "f64", B); nx = gm.spec.nx
    DZ, DC, G = synthetic("ant", "f64", H, B, seed=3)
    clean_e, clean_t, clean_z = data_adjoint(gm, DZ, DC, G)
    DZn, DCn = DZ.copy(), DC.copy(); DZn[2, 1] = np.nan; DCn[2, 1] = np.nan
    status = np.zeros((H, B), np.int32); status[2, 1] = 1
    gte, gt, gz = data_adjoint(gm, DZn, DCn, G, status=status)
    assert np.isfinite(gte).all() and np.isfinite(gt).all() and np.isfinite(gz).all()
    ra, rz = recursion(DZn, DCn, G, status)
    aa, az = recursion(np.abs(DZ), np.abs(DC), np.abs(G), status)
    check(gz, rz, az, H, nx, False, what="gz"); check(gte, ra, aa, H, nx, False, what="gtheta_env"); check_sum(gt, ra, aa, H, nx, False)
    assert not np.array_equal(gte[1], clean_e[1])
    for b in (0, 2, 3):
        assert np.array_equal(gte[b], clean_e[b]) and np.array_equal(gz[b], clean_z[b])
    # ... and with status all zero the result is the one without a status buffer
    ze, zt, zz = data_adjoint(gm, DZ, DC, G, status=np.zeros((H, B), np.int32))
    assert np.array_equal(ze, clean_e) and np.array_equal(zt, clean_t) and np.array_equal(zz, clean_z)


def test_deterministic_and_independent_of_the_batch():
    """4. fixed summation orders: two runs agree bit for bit (the shared sum included), and an environment run alone (B = 1) agrees with its place
    in a batch of 65 in gtheta_env and gz"""
    H, B = 7, 65
    DZ, DC, G = synthetic("ant", "f64", H, B)
    gm = _handle("ant", "f64", B)
    gte, gt, gz = data_adjoint(gm, DZ, DC, G)
    gte2, gt2, gz2 = data_adjoint(gm, DZ, DC, G)
    assert np.array_equal(gte, gte2) and np.array_equal(gt, gt2) and np.array_equal(gz, gz2)
    g1 = _handle("ant", "f64", 1)
    for b in (0, 32, 64):
        se, _, sz = data_adjoint(g1, DZ[:, b:b + 1], DC[:, b:b + 1], G[:, b:b + 1])
        assert np.array_equal(se[0], gte[b]) and np.array_equal(sz[0], gz[b]), b


def record(gm, z0, U, H, with_dc=True):
    """dojo_rollout_data_record_dev (with_dc) or dojo_rollout_record_dev on torch tensors -> (rc, Z, status, DZ [H,B,c,r], DU [H,B,c,r], DC [H,B,c,r])"""
    s, B = gm.spec, gm.batch
    tdt = torch.float32 if gm.dtype_code else torch.float64
    Z = torch.empty((H, B, s.nz), dtype=tdt, device="cuda"); st = torch.empty((H, B), dtype=torch.int32, device="cuda")
    DZ = torch.empty((H, B, s.nx, s.nx), dtype=tdt, device="cuda"); DU = torch.empty((H, B, max(s.nu, 1), s.nx), dtype=tdt, device="cuda")
    DC = torch.full((H, B, max(_nth(gm), 1), s.nx), 77.0, dtype=tdt, device="cuda")
    z0d, Ud = dev(z0.astype(gm.np_dtype)), dev(None if U is None else U.astype(gm.np_dtype))
    if with_dc:
        rc = api.lib().dojo_rollout_data_record_dev(gm.h, api.addr(z0d), api.addr(Ud), int(H), api.addr(Z), api.addr(st), api.addr(DZ), api.addr(DU), api.addr(DC), api.torch_stream())
    else:
        rc = api.lib().dojo_rollout_record_dev(gm.h, api.addr(z0d), api.addr(Ud), int(H), api.addr(Z), api.addr(st), api.addr(DZ), api.addr(DU), api.torch_stream())
    torch.cuda.synchronize()
    return rc, Z.cpu().numpy(), st.cpu().numpy(), DZ.cpu().numpy(), DU.cpu().numpy()[:, :, :s.nu], DC.cpu().numpy()[:, :, :_nth(gm)]


_stepwise = {}


def ant_stepwise(B, H):
    """Ant f64 through the EXISTING paths, once per shape: rollout, and step(with_gradient) + gradients() + contact_gradients() from the rollout's
    states, transposed to the device layout [B, column, row]"""
    if (B, H) not in _stepwise:
        spec = _spec("ant")
        z0, u = d.synthetic_inputs(spec, B)
        rng = np.random.default_rng(5)
        U = np.stack([u * rng.uniform(0.5, 1.0) for _ in range(H)])
        gm = _handle("ant", "f64", B)
        Z, st = gm.rollout(z0, U)
        DZ, DU, DC = [], [], []
        for k in range(H):
            zn, sk, _ = gm.step(z0 if k == 0 else Z[k - 1], U[k], with_gradient=True)
            assert np.array_equal(zn, Z[k]) and np.array_equal(sk, st[k])
            dz, du = gm.gradients()
            dc = gm.contact_gradients()
            DZ.append(dz.transpose(0, 2, 1)); DU.append(du.transpose(0, 2, 1)); DC.append(dc.transpose(0, 2, 1))
        _stepwise[(B, H)] = (z0, U, Z, st, np.stack(DZ), np.stack(DU), np.stack(DC))
    return _stepwise[(B, H)]


@pytest.mark.parametrize("B,H", [(64, 4), (600, 3)])
def test_record_is_the_stepwise_path(B, H):
    """5. dojo_rollout_data_record_dev: states, status and Jacobians of dojo_rollout_record_dev bit for bit, and on solved steps the contact-data
    columns of dojo_step + dojo_contact_gradients from the rollout's states, bit for bit (600 environments: several environment groups)"""
    z0, U, Z, st, DZ, DU, DC = ant_stepwise(B, H)
    gm = _handle("ant", "f64", B)
    rc0, Z0, s0, DZ0, DU0, _ = record(gm, z0, U, H, with_dc=False)
    rc, Zr, sr, DZr, DUr, DCr = record(gm, z0, U, H)
    assert rc0 == 0 and rc == 0
    assert np.array_equal(Zr, Z0) and np.array_equal(sr, s0) and np.array_equal(Zr, Z) and np.array_equal(sr, st)
    ok = sr == 0                                                             # (what a failed step leaves in its Jacobians is nobody's contract)
    assert ok.mean() >= 0.9
    assert np.array_equal(DZr[ok], DZ0[ok]) and np.array_equal(DUr[ok], DU0[ok])
    assert np.isfinite(DCr[ok]).all() and np.abs(DCr[ok]).max() > 0
    assert np.array_equal(DCr[ok], DC[ok])


def _theta_spec(name, theta):
    """the mechanism `name` created with the contact data theta [Nc, 5]"""
    spec = _spec(name)
    for c, t in zip(spec.contacts, np.asarray(theta, np.float64)):
        c.friction_coefficient = float(t[0]); c.radius = float(t[1]); c.origin = np.array(t[2:5], np.float64)
    return spec


@pytest.mark.parametrize("name", ["sphere", "block"])
def test_set_contact_data_is_a_fresh_handle(name):
    """6. after set_contact_data(theta') a handle steps and rolls out as one created with theta', bit for bit; contact_data() returns theta';
    the solution of an earlier differentiable step no longer serves contact_gradients()"""
    B, H = 8, 4
    spec = _spec(name)
    z0, u = floor_states(spec, B)
    U = np.stack([u] * H)
    gm = api.BatchedMechanism(spec, B, dtype="f64")
    fresh = None
    try:
        th0 = gm.contact_data()
        assert th0.shape == (len(spec.contacts), 5)
        assert np.array_equal(th0, np.array([[c.friction_coefficient, c.radius, *c.origin] for c in spec.contacts]))
        rng = np.random.default_rng(17)
        th1 = th0.copy(); th1[:, 0] = 0.35; th1[:, 1] += 0.002; th1[:, 2:] += 0.001 * rng.standard_normal(th1[:, 2:].shape)
        Zold, _ = gm.rollout(z0, U)
        gm.step(z0, u, with_gradient=True)
        gm.contact_gradients()
        gm.set_contact_data(th1)
        assert np.array_equal(gm.contact_data(), th1)
        with pytest.raises(api.DojoError):
            gm.contact_gradients()
        fresh = api.BatchedMechanism(_theta_spec(name, th1), B, dtype="f64")
        zs, ss, its = gm.step(z0, u); zf, sf, itf = fresh.step(z0, u)
        assert np.array_equal(zs, zf) and np.array_equal(ss, sf) and np.array_equal(its, itf)
        Zs, sts = gm.rollout(z0, U); Zf, stf = fresh.rollout(z0, U)
        assert np.isfinite(Zs).all() and (sts == 0).mean() >= 0.9
        assert np.array_equal(Zs, Zf) and np.array_equal(sts, stf)
        assert not np.array_equal(Zs, Zold)                                  # (the data did change the rollout)
        # a negative radius: INVALID, and nothing changed
        bad = th1.copy(); bad[0, 1] = -0.1
        assert api.lib().dojo_set_contact_data(gm.h, api.addr(bad)) == INVALID and "dojo_set_contact_data" in gm.last_error()
        assert np.array_equal(gm.contact_data(), th1)
    finally:
        gm.close()
        if fresh is not None:
            fresh.close()


def test_set_contact_data_refuses_impact_friction():
    """6b. an ImpactContact has no friction coefficient: anything but 0 is UNSUPPORTED, 0 is accepted"""
    spec = d.get_mechanism("sphere", contact_type="impact")
    gm = api.BatchedMechanism(spec, 2, dtype="f64")
    try:
        th = gm.contact_data()
        assert th[0, 0] == 0.0
        th[0, 0] = 0.3
        assert api.lib().dojo_set_contact_data(gm.h, api.addr(th)) == UNSUPPORTED and "ImpactContact" in gm.last_error()
        th[0, 0] = 0.0; th[0, 1] = 0.4
        gm.set_contact_data(th)
        assert np.array_equal(gm.contact_data(), th)
    finally:
        gm.close()


def test_rollout_data_gradients_end_to_end():
    """7. the host entry on real Jacobians: against the recursion over the Jacobians of the existing step / gradients / contact_gradients path,
    cut at the device's own status; gU is rollout_gradients' bit for bit"""
    B, H = 64, 4
    z0, U, Z, st, DZ, DU, DC = ant_stepwise(B, H)
    gm = _handle("ant", "f64", B); nx = gm.spec.nx
    G = np.random.default_rng(9).standard_normal((H, B, nx))
    Zg, sg, gth, gte, gU, gz = gm.rollout_data_gradients(z0, U, G, per_env=True)
    assert np.array_equal(Zg, Z) and np.array_equal(sg, st)
    ra, rz = recursion(DZ, DC, G, st)
    aa, az = recursion(np.abs(DZ), np.abs(DC), np.abs(G), st)
    check(gz, rz, az, H, nx, False, what="gz")
    check(gte.reshape(B, -1), ra, aa, H, nx, False, what="gtheta_env")
    check_sum(gth.reshape(-1), ra, aa, H, nx, False)
    assert np.abs(batch_sum(ra)).max() > 0
    _, _, gU0, gz0 = gm.rollout_gradients(z0, U, G)
    assert np.array_equal(gU, gU0) and np.array_equal(gz, gz0) and np.abs(gU0).max() > 0
    _, _, gth1, gte1, _, _ = gm.rollout_data_gradients(z0, U, G)
    assert gte1 is None and np.array_equal(gth1, gth)


def attitude_tangent(W):
    """a state-space cotangent [.., 13 Nb] whose quaternion entries are zero, in tangent coordinates [.., 12 Nb]"""
    w = W.reshape(W.shape[:-1] + (-1, 13))
    return np.concatenate([w[..., 0:6], np.zeros(w.shape[:-1] + (3,)), w[..., 10:13]], -1).reshape(W.shape[:-1] + (-1,))


def fd_data_chain(name, z0, B, H, ndir_random=2, eps=1e-6, axes=True):
    """-> dict: per direction d in theta space, over the counted environments, the worst |x - fd| / max(1, |an|) of x = the new path's <gtheta_env, d>
    and of x = the EXISTING per-step chain's (step + gradients + contact_gradients, dc <- dth + dz dc in NumPy, as
    examples/sphere_system_identification_device.py), fd = central differences of the existing rollout under set_contact_data(theta +- eps d);
    the worst excess of |new - chain| over the rounding bound; the fraction of environments counted"""
    spec = _spec(name)
    gm = api.BatchedMechanism(spec, B, dtype="f64", opts=d.SolverOptions(rtol=1e-9, btol=1e-9))
    try:
        gm.set_gradient_mode(api.GRAD_CONSISTENT)
        nx, nth = spec.nx, 5 * len(spec.contacts)
        th0 = gm.contact_data()
        rng = np.random.default_rng(21)
        W = rng.standard_normal((H, B, spec.Nb, 13)); W[..., 6:10] = 0.0; W = W.reshape(H, B, spec.nz)      # linear in the x, v, omega components
        Z0, st0, _, gte, _, _ = gm.rollout_data_gradients(z0, None, W, cot_space="state", per_env=True)
        gte = gte.reshape(B, nth)
        # the existing chain, forward, from the rollout's own states
        Gt = attitude_tangent(W)
        dc = np.zeros((B, nx, nth)); chain = np.zeros((B, nth)); achain = np.zeros((B, nth)); adc = np.zeros((B, nx, nth))
        same = np.ones(B, bool)                                              # the stepwise path reproduces the rollout (bit for bit where it is solved)
        for k in range(H):
            zn, sk, _ = gm.step(z0 if k == 0 else Z0[k - 1], with_gradient=True)
            same &= (zn == Z0[k]).all(1) & (sk == st0[k])
            dz, _ = gm.gradients(); dth = gm.contact_gradients()
            dc = dth + dz @ dc; adc = np.abs(dth) + np.abs(dz) @ adc
            chain += np.einsum("br,brc->bc", Gt[k], dc); achain += np.einsum("br,brc->bc", np.abs(Gt[k]), adc)
        solved = (st0 == 0).all(0) & same
        excess = float((np.abs(gte - chain) - bound(H, nx, 3, achain, chain, False))[solved].max()) if solved.any() else 0.0
        dirs = []
        if axes:
            e0 = np.zeros((nth // 5, 5)); e0[:, 0] = 1.0; e1 = np.zeros((nth // 5, 5)); e1[:, 1] = 1.0
            dirs += [e0, e1]                                                  # along friction, along radius
        dirs += [rng.standard_normal((nth // 5, 5)) for _ in range(ndir_random)]
        counted = solved.copy()
        fds = []
        for D in dirs:
            gm.set_contact_data(th0 + eps * D); Zp, sp = gm.rollout(z0, steps=H)
            gm.set_contact_data(th0 - eps * D); Zm, sm = gm.rollout(z0, steps=H)
            counted &= (sp == 0).all(0) & (sm == 0).all(0)
            fds.append((W * (Zp - Zm)).sum(axis=(0, 2)) / (2 * eps))
        gm.set_contact_data(th0)
        err_new = err_chain = 0.0
        for D, fd in zip(dirs, fds):
            an_new = gte @ D.reshape(-1); an_chain = chain @ D.reshape(-1)
            scale = np.maximum(1.0, np.abs(an_chain))
            if counted.any():
                err_new = max(err_new, float((np.abs(an_new - fd) / scale)[counted].max()))
                err_chain = max(err_chain, float((np.abs(an_chain - fd) / scale)[counted].max()))
        return dict(err_new=err_new, err_chain=err_chain, excess=excess, frac=float(counted.mean()), gmax=float(np.abs(gte).max()))
    finally:
        gm.close()


def test_chain_is_the_derivative_of_the_rollout():
    """8. a sphere (friction coefficient 0.2, radius 0.5) sliding on the floor: x = (0, 0, r), horizontal velocity 1 .. 3 m/s per environment, no spin.
    It decelerates with mu g = 1.96 m/s^2 and would only start to roll after (2/7) |v| / (mu g) >= 0.146 s, so over H = 6 steps of 0.01 s it slides:
    no stick / slip switch, no lift-off (checked with the CPU oracle at theta and at theta +- 2e-6: deceleration mu g to 2e-3 in every step of every
    environment, slip velocity at the contact point >= 0.58 m/s).  GRAD_CONSISTENT, rtol = btol = 1e-9, B = 8, loss linear in the x, v, omega
    components; central differences with eps = 1e-6 along friction, along radius and along two random 5-vectors.

    The yardstick is the EXISTING per-step chain (dojo_step + dojo_gradients + dojo_contact_gradients, chained forward in NumPy as the system
    identification example does), computed in the same test: the new path must agree with it to the rounding bound of test 1, the chain itself must
    be within 1e-3 of the differences (else the inputs cross a mode switch), and the new path's finite-difference error must be <= 10 x the chain's,
    rounded up to a power of ten (ten: the dependence of the differences' own error on eps).
    Measured on an MI355X: finite-difference error of the existing chain 2.965e-04, of the new path 2.965e-04 (the size of both is
    the solver tolerance over eps, 1e-9 / 1e-6), so the assertion is <= 10 x 1e-3; new path against the chain: 1.3e-13 inside the rounding bound; all 8
    environments counted.  Ant (printed, not asserted): 2.9e-3 for both."""
    B, H = 8, 6
    out = fd_data_chain("sliding_sphere", sliding_states(_spec("sliding_sphere"), B), B, H)
    print("sliding sphere: FD error of the new path %.3e, of the existing chain %.3e (relative, max(1, |an|)); new - chain beyond the rounding bound: %.3e; "
          "%.0f %% of the environments; max |gtheta_env| %.3e" % (out["err_new"], out["err_chain"], out["excess"], 100 * out["frac"], out["gmax"]))
    assert out["frac"] >= 0.9
    assert out["gmax"] > 0
    assert out["excess"] <= 0.0
    assert out["err_chain"] <= 1e-3
    tol = 10.0 * 10.0 ** math.ceil(math.log10(max(out["err_chain"], 1e-300)))
    assert out["err_new"] <= tol
    z0, _ = d.synthetic_inputs(_spec("ant"), B)
    ant = fd_data_chain("ant", z0, B, H, axes=False)
    print("ant (not asserted): FD error of the new path %.3e, of the existing chain %.3e, %.0f %% of the environments" % (ant["err_new"], ant["err_chain"], 100 * ant["frac"]))


def sliding_states(spec, B):
    rng = np.random.default_rng(33)
    ang = rng.uniform(0.0, 2.0 * np.pi, B); speed = np.linspace(1.0, 3.0, B)
    z = np.zeros((B, 13)); z[:, 2] = spec.contacts[0].radius; z[:, 3] = speed * np.cos(ang); z[:, 4] = speed * np.sin(ang); z[:, 6] = 1.0
    return z


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
    """9. torch.autograd through differentiable_data_rollout (block with four corners, fp32): theta's gradient is the host entry's gtheta rounded
    once more (fp32 -> the fp64 of theta: exact), U's is gU bit for bit, z0's the lifted gz to within one unit in the last place"""
    from dojo_amd.autograd import differentiable_data_rollout
    B, H = 16, 5
    spec = _spec("block")
    gm = _handle("block", "f32", B)
    z0, u = floor_states(spec, B)
    rng = np.random.default_rng(13)
    U = np.stack([u * rng.uniform(0.5, 1.0) for _ in range(H)]).astype(np.float32); z0 = z0.astype(np.float32)
    W = rng.standard_normal((H, B, spec.nz)).astype(np.float32)
    th = gm.contact_data()
    Zh, sh, gth, _, gU, gz = gm.rollout_data_gradients(z0, U, W, cot_space="state")
    zt = dev(z0).requires_grad_(True); Ut = dev(U).requires_grad_(True)
    for theta in (torch.from_numpy(th.copy()).requires_grad_(True), dev(th).requires_grad_(True)):      # CPU and device
        Z = differentiable_data_rollout(gm, zt, Ut, theta)
        assert Z.status.dtype == torch.int32 and not Z.status.requires_grad
        gtt, gUt, gzt = torch.autograd.grad((Z * dev(W)).sum(), [theta, Ut, zt])
        torch.cuda.synchronize()
        assert np.array_equal(Z.detach().cpu().numpy(), Zh) and np.array_equal(Z.status.cpu().numpy(), sh)
        assert gtt.dtype == torch.float64 and gtt.device == theta.device and tuple(gtt.shape) == th.shape
        assert np.array_equal(gtt.cpu().numpy(), gth.astype(np.float64)) and np.abs(gth).max() > 0
        assert np.array_equal(gUt.cpu().numpy(), gU) and np.abs(gU).max() > 0
        ref = lift(gz, z0, True).astype(np.float32)                          # rounded once, like the wrapper's
        got = gzt.cpu().numpy()
        assert got.dtype == np.float32 and np.abs(ref).max() > 0
        assert np.all(np.abs(got - ref) <= np.spacing(np.abs(ref)))            # one unit in the last place of every entry, nothing absolute


def test_argument_errors():
    """10. every argument error of the two device entries: DOJO_ERR_INVALID, a message on the handle naming the entry point, nothing launched (the
    outputs keep their fill); mechanisms without contact-data gradients: DOJO_ERR_UNSUPPORTED before any launch"""
    H, B = 2, 3
    gm = _handle("block", "f64", B); s = gm.spec; nth = _nth(gm)
    DZ, DC, G = (dev(a) for a in synthetic("block", "f64", H, B))
    Z = torch.zeros((H, B, s.nz), dtype=torch.float64, device="cuda")
    fill = lambda *shape: torch.full(shape, 77.0, dtype=torch.float64, device="cuda")
    gte, gt, gz = fill(B, nth), fill(nth), fill(B, s.nx)
    untouched = lambda: bool((gte == 77.0).all() and (gt == 77.0).all() and (gz == 77.0).all())
    bad = {"H < 1": dict(H=0), "DZ NULL": dict(DZ=None), "DC NULL": dict(DC=None), "G NULL": dict(G=None), "cot_space 1 without Z": dict(cot_space=1, Z=None),
           "no output": dict(gte=None, gt=None, gz=None)}
    for what, kw in bad.items():
        a = dict(H=H, DZ=DZ, DC=DC, G=G, cot_space=0, Z=Z, status=None, gte=gte, gt=gt, gz=gz); a.update(kw)
        rc = data_adjoint_raw(gm, a.pop("H"), a.pop("DZ"), a.pop("DC"), a.pop("G"), **a)
        torch.cuda.synchronize()
        assert rc == INVALID, what
        msg = gm.last_error()
        assert "dojo_rollout_data_adjoint_dev" in msg, (what, msg)
        assert untouched(), what
    # the kernel reads DZ and DC in 16-byte pieces: a pointer into the middle of a piece is refused
    for what, kw in {"DZ unaligned": dict(DZ=DZ.view(-1)[1:]), "DC unaligned": dict(DC=DC.view(-1)[1:])}.items():
        a = dict(H=1, DZ=DZ, DC=DC, G=G, cot_space=0, Z=Z, status=None, gte=gte, gt=gt, gz=gz); a.update(kw)
        rc = data_adjoint_raw(gm, a.pop("H"), a.pop("DZ"), a.pop("DC"), a.pop("G"), **a)
        torch.cuda.synchronize()
        assert rc == INVALID and "16-byte" in gm.last_error() and "dojo_rollout_data_adjoint_dev" in gm.last_error(), (what, gm.last_error())
        assert untouched(), what
    # the record entry: its own argument errors ...
    z0 = dev(np.tile(d.initialize(s), (B, 1)))
    Zr = fill(H, B, s.nz); DZr = fill(H, B, s.nx, s.nx); DUr = fill(H, B, s.nu, s.nx); DCr = fill(H, B, nth, s.nx)
    rec = lambda **kw: api.lib().dojo_rollout_data_record_dev(gm.h, api.addr(kw.get("z0", z0)), None, int(kw.get("H", H)), api.addr(kw.get("Z", Zr)), None,
                                                              api.addr(kw.get("DZ", DZr)), api.addr(kw.get("DU", DUr)), api.addr(DCr), api.torch_stream())
    for what, kw in {"H < 1": dict(H=0), "z0 NULL": dict(z0=None), "Z NULL": dict(Z=None), "DZ NULL": dict(DZ=None), "DU NULL": dict(DU=None)}.items():
        rc = rec(**kw)
        torch.cuda.synchronize()
        assert rc == INVALID and "dojo_rollout_data_record_dev" in gm.last_error(), (what, gm.last_error())
        assert bool((Zr == 77.0).all() and (DZr == 77.0).all() and (DUr == 77.0).all() and (DCr == 77.0).all()), what
    # ... and a mechanism it has no contact-data columns for
    spec = d.get_mechanism("sphere", contact_type="linear")
    gl = api.BatchedMechanism(spec, 4, dtype="f64")
    try:
        z0l = np.tile(d.initialize(spec), (4, 1))
        rc, _, _, _, _, DCl = record(gl, z0l, None, 2)
        assert rc == UNSUPPORTED and "LinearContact" in gl.last_error() and "dojo_rollout_data_record_dev" in gl.last_error()
        assert (DCl == 77.0).all()
        with pytest.raises(api.DojoError):
            gl.rollout_data_gradients(z0l, None, np.zeros((2, 4, spec.nx)))
        assert "dojo_rollout_data_gradients" in gl.last_error()
    finally:
        gl.close()


# ---------------------------------------------------------------- the memory refusal of the four *_gradients host entries ----------------------------------------------------------------
def _gradients_call(entry, gm, spec, H, z0, G, theta, status, gz):
    """one raw call of a *_gradients host entry on host arrays: no controls, tangent-space cotangents, a shared policy on input 0 (theta: W, or the network's
    parameters for the widths [2 nu, 3, 1]); of the outputs, status and gz alone are asked for"""
    L, p, nobs = api.lib(), api.addr, 2 * spec.nu
    if entry == "dojo_rollout_gradients":
        return L.dojo_rollout_gradients(gm.h, p(z0), None, H, p(G), 0, None, p(status), None, p(gz))
    if entry == "dojo_rollout_data_gradients":
        return L.dojo_rollout_data_gradients(gm.h, p(z0), None, H, p(G), 0, None, p(status), None, None, None, p(gz))
    if entry == "dojo_rollout_policy_gradients":
        pol = api.DojoPolicy(theta.ctypes.data, None, None, None, None, 0, 0, 1, 0, 0, 0)
        return L.dojo_rollout_policy_gradients(gm.h, p(z0), C.byref(pol), H, p(G), 0, None, None, None, None, None, p(status), None, None, None, p(gz))
    pol = api.mlp_policy_struct(theta.ctypes.data, None, None, None, 0, 0, [nobs, 3, 1])
    return L.dojo_rollout_mlp_gradients(gm.h, p(z0), C.byref(pol), H, p(G), 0, None, None, None, None, None, p(status), None, None, p(gz))


@pytest.mark.parametrize("entry", ["dojo_rollout_gradients", "dojo_rollout_data_gradients", "dojo_rollout_policy_gradients", "dojo_rollout_mlp_gradients"])
def test_record_larger_than_the_device_is_refused(entry):
    """A horizon whose record -- H B nx (nx + nu) scalars, plus 5 Nc columns for the data entry -- is at least twice the device's total memory: the entry
    refuses with DOJO_ERR_INVALID before it reads, allocates or launches anything (the host arrays are one-element dummies), names itself, the record's byte
    count and the free device memory; the same handle then completes the entry at H = 2.  H stays below 2^31 and the record below 2^50, so that no size of
    the call (none exceeds the record) comes near 2^63."""
    B, w = 3, 8
    data = entry == "dojo_rollout_data_gradients"
    spec = d.get_mechanism("sphere") if data else d.get_mechanism("cartpole")
    nx, nu, Nc = spec.nx, spec.nu, len(spec.contacts)
    assert Nc > 0 or not data
    per_step = B * nx * (nx + nu + (5 * Nc if data else 0)) * w
    total = torch.cuda.mem_get_info()[1]
    H = -(-2 * total // per_step)
    record = H * per_step
    assert record >= 2 * total and H < 2 ** 31 and record < 2 ** 50
    theta = np.zeros(2 * nu if entry == "dojo_rollout_policy_gradients" else api.mlp_sizes([2 * nu, 3, 1])[0])
    gm = api.BatchedMechanism(spec, B, dtype="f64")
    try:
        one, gz1 = np.zeros(1), np.full(1, 77.0)
        rc = _gradients_call(entry, gm, spec, H, one, one, theta[:1], None, gz1)
        err = gm.last_error()
        print(entry, "H", H, "record", record, "rc", rc, err)
        assert rc == INVALID and entry in err and str(record) in err and "free device memory" in err, (rc, err)
        assert gz1[0] == 77.0
        z0 = floor_states(spec, B)[0] if data else d.synthetic_inputs(spec, B)[0]
        status = np.full((2, B), -77, dtype=np.int32); gz = np.full((B, nx), np.nan)
        rc = _gradients_call(entry, gm, spec, 2, z0, np.ones((2, B, nx)), theta, status, gz)
        assert rc == 0, (rc, gm.last_error())
        assert (status != -77).all() and np.isfinite(gz).all()
    finally:
        gm.close()
