"""Reverse mode through closed-loop rollouts on the GPU: dojo_rollout_policy_adjoint_dev against the recursion it implements (NumPy fp64 on the same
values), dojo_observation_jacobian_dev against finite differences of the oracle's map, dojo_rollout_policy_record_dev against the two existing
paths, dojo_rollout_policy_gradients end to end, the chain against finite differences of the closed loop, the shared policy, and the torch.autograd
wrapper.

The recursion, per environment, with ohat_k = (OBS[k] - mean) .* scale, M_k the observation Jacobian at the state step k starts from:
    lambda <- g_{H-1} + M_H^T GO_H
    for k = H-1 .. 0:  failed step: lambda <- 0
                       gu = DU_k^T lambda + GU_k -> gU[k];  a = gu[act_off : act_off + na];  gbias += a;  gW += a ohat_k^T
                       go = scale .* (W^T a) + GO_k;  lambda = DZ_k^T lambda + M_k^T go (+ g_{k-1} if k > 0)
    gz <- lambda

Error bound of the kernel tests (elementwise; Higham, Accuracy and Stability of Numerical Algorithms, 3.1: two summation orders of an n-term dot
product differ by at most gamma_n sum |x_i y_i| each).  `abs_` is the same recursion run on absolute values, with |ohat| replaced by
(|o| + |mean|) |scale|.  The longest chain of one step of the kernel, counted in its source (csrc/dojo_policy_adjoint.hpp): lambda + g (1), the
nx-term column product (nx), a = gu + GU (1), the na-term W^T a (na), the scale product and the addition of GO (2), the M^T go sum over the
rows that touch a body (at most nobs) and its addition to lambda (1); the accumulators add ohat's subtraction and product and one
multiply-add (3): nx + nobs + na + 8, the count the bound was specified with.  Ten more where the state cotangent is first pulled back from
state coordinates.  So
    |out - ref| <= 2 (H n_step + n_red) 2^-53 abs_   (+ 2^-23 |ref| for fp32 outputs: one rounding of the result, a whole ulp)
with n_red = B for the outputs of a shared policy (the sum over the batch) and 0 otherwise."""
import ctypes as C

import numpy as np
import pytest
import torch

import dojo_amd as d
from dojo_amd import api, coords
from gpu_util import dev, same, tdt_of

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -2
K_REFERENCE = np.array([-0.948838, -2.54837, 48.6627, 10.871])      # docs/src/creating_simulation/define_controller.md:23
# mechanism -> (first driven input, driven inputs)
ACT = {"pendulum": (0, 1), "cartpole": (0, 1), "ant": (6, 8), "atlas": (6, 30)}
OUTS = ("gW", "gbias", "gU", "gz")


def _spec(name):
    if name == "ant":
        return d.baseline_config(3)
    if name == "atlas":
        return d.baseline_config(5)
    if name == "fixed3":
        return d.get_npendulum(num_bodies=3, base_joint_type="Fixed", rest_joint_type="Fixed")
    if name == "sphere_linear":
        return d.get_sphere(contact_type="linear")
    return d.get_mechanism(name)


_handles = {}


def _handle(name, dtype, B, tight=False):
    """one handle per (mechanism, dtype, batch, options) for the whole module; tight: rtol = btol = 1e-9 and GRAD_CONSISTENT"""
    key = (name, dtype, B, tight)
    if key not in _handles:
        gm = api.BatchedMechanism(_spec(name), B, dtype=dtype, opts=d.SolverOptions(rtol=1e-9, btol=1e-9) if tight else None)
        if tight:
            gm.set_gradient_mode(api.GRAD_CONSISTENT)
        _handles[key] = gm
    return _handles[key]


def teardown_module(module):
    for gm in _handles.values():
        gm.close()
    _handles.clear()


def sweep_raw(gm, H, t, per_env, act_off, na, cot_space=0, contact_forces=0):
    """dojo_rollout_policy_adjoint_dev on a dict of torch tensors (missing / None = NULL) -> return code"""
    g = lambda k: api.addr(t.get(k))
    pol = api.DojoPolicy(g("W"), None, g("mean"), g("scale"), None, int(per_env), int(act_off), int(na), int(contact_forces), 0, 0)
    a = api.DojoPolicyAdjoint(g("DZ"), g("DU"), g("OBS"), g("status"), g("z0"), g("Z"), g("M"), g("G"), g("G_u"), g("G_obs"),
                              g("gW"), g("gbias"), g("gU"), g("gz"), int(cot_space), 0)
    return api.lib().dojo_rollout_policy_adjoint_dev(gm.h, C.byref(pol), int(H), C.byref(a), api.torch_stream())


def out_tensors(gm, H, per_env, na, fill=float("nan")):
    s, B, tdt = gm.spec, gm.batch, tdt_of(gm)
    nobs = 2 * s.nu
    f = lambda shape: torch.full(shape, fill, dtype=tdt, device="cuda")
    return {"gW": f((B, na, nobs) if per_env else (na, nobs)), "gbias": f((B, na) if per_env else (na,)), "gU": f((H, B, s.nu)), "gz": f((B, s.nx))}


def sweep(gm, H, inp, per_env, act_off, na, cot_space=0, outs=None):
    """NumPy in, NumPy out (dict over OUTS); the outputs start as NaN so that an entry the kernels leave out shows.
    outs: the caller's own device tensors instead (a missing key = NULL, and missing from the result)"""
    t = {k: dev(v) for k, v in inp.items()}
    t.update(out_tensors(gm, H, per_env, na) if outs is None else outs)
    api._chk(sweep_raw(gm, H, t, per_env, act_off, na, cot_space))
    torch.cuda.synchronize()
    return {k: t[k].cpu().numpy() for k in OUTS if t.get(k) is not None}


def recursion(spec, inp, act_off, na, absolute=False):
    """the reference: fp64 NumPy on a dict with DZ [H,B,c,r], DU [H,B,c,r], OBS [H+1,B,nobs], M compact [H+1,B,nobs,24], W [B,na,nobs] or [na,nobs],
    G [H,B,nx] tangent and optional mean, scale, G_u, G_obs, status.  A failed step's Jacobians are not touched; the parent columns of origin
    joints never leave the compact M.  absolute: |ohat| <- (|o| + |mean|) |scale| (the inputs are then absolute values).
    -> dict over OUTS, gW / gbias per environment."""
    f = lambda k: None if inp.get(k) is None else np.asarray(inp[k], np.float64)
    DZ, DU, OBS, G, GU, GO, W = f("DZ"), f("DU"), f("OBS"), f("G"), f("G_u"), f("G_obs"), f("W")
    H, B, nx = G.shape
    nobs = OBS.shape[2]
    Md = coords.dense_observation_jacobian(spec, f("M").reshape((H + 1) * B, nobs, 24)).reshape(H + 1, B, nobs, nx)
    mean = np.zeros(nobs) if inp.get("mean") is None else f("mean")
    scale = np.ones(nobs) if inp.get("scale") is None else f("scale")
    status = inp.get("status")
    if W.ndim == 2:
        W = np.broadcast_to(W, (B,) + W.shape)
    gW = np.zeros((B, na, nobs)); gb = np.zeros((B, na)); gU = np.zeros((H, B, DU.shape[2]))
    lam = G[H - 1].copy()
    if GO is not None:
        lam = lam + np.einsum("bro,br->bo", Md[H], GO[H])
    for k in range(H - 1, -1, -1):
        ok = np.ones(B, bool) if status is None else (np.asarray(status)[k] == 0)
        gu = np.zeros((B, DU.shape[2])); new = np.zeros((B, nx))
        gu[ok] = np.einsum("bcr,br->bc", DU[k][ok], lam[ok]); new[ok] = np.einsum("bcr,br->bc", DZ[k][ok], lam[ok])
        if GU is not None:
            gu = gu + GU[k]
        gU[k] = gu
        a = gu[:, act_off:act_off + na]
        ohat = (OBS[k] + mean) * scale if absolute else (OBS[k] - mean) * scale
        gb += a; gW += a[:, :, None] * ohat[:, None, :]
        go = scale * np.einsum("bij,bi->bj", W, a)
        if GO is not None:
            go = go + GO[k]
        lam = new + np.einsum("bro,br->bo", Md[k], go)
        if k > 0:
            lam = lam + G[k - 1]
    return {"gW": gW, "gbias": gb, "gU": gU, "gz": lam}


def absolute(inp):
    return {k: (v if (v is None or k == "status") else np.nan_to_num(np.abs(np.asarray(v, np.float64)), nan=0.0)) for k, v in inp.items()}


def check(out, ref, abs_, H, n_step, f32, n_red=0, what=""):
    err = np.abs(out.astype(np.float64) - ref)
    lim = 2.0 * (H * n_step + n_red) * 2.0 ** -53 * abs_ + (2.0 ** -23 * np.abs(ref) if f32 else 0.0)
    assert np.isfinite(out).all(), what
    worst = (err - lim).max()
    assert worst <= 0.0, "%s: error exceeds the bound by %.3e (max error %.3e, max |ref| %.3e)" % (what, worst, err.max(), np.abs(ref).max())


def check_all(spec, out, inp, act_off, na, H, f32, per_env=True, extra=0, abs_G=None):
    """every output in `out` against the recursion on inp.  abs_G: what stands for |G| in the bound's recursion where G was pulled back from state
    coordinates (the sum of the magnitudes of the terms of every entry, pull_back's second result)"""
    nx, nobs = spec.nx, 2 * spec.nu
    ainp = absolute(inp) if abs_G is None else dict(absolute(inp), G=abs_G)
    ref, abs_ = recursion(spec, inp, act_off, na), recursion(spec, ainp, act_off, na, absolute=True)
    n_step = nx + nobs + na + 8 + extra
    for k in out:
        shared = (not per_env) and k in ("gW", "gbias")
        r, a = (ref[k].sum(0), abs_[k].sum(0)) if shared else (ref[k], abs_[k])
        check(out[k], r, a, H, n_step, f32, n_red=spec_batch(inp) if shared else 0, what=k)
    return ref


def spec_batch(inp):
    return np.asarray(inp["G"]).shape[1]


def origin_rows(spec):
    """rows of the observation whose joint sits on the origin"""
    rows, r = [], 0
    for j in spec.joints:
        if j.parent < 0:
            rows += list(range(r, r + 2 * j.nu))
        r += 2 * j.nu
    return rows


_inputs = {}


def synthetic(name, dtype, H, B, seed=7):
    """Scales chosen so that |lambda| neither grows nor decays by more than about 10x per step: DZ ~ 1.3 N(0,1) / sqrt(nx) (a random matrix of
    spectral radius about 1.3), DU ~ N(0,1) / sqrt(nx) (|gu| about |lambda|), W ~ N(0,1) / sqrt(na) (|go| about |a|), M ~ N(0,1) / sqrt(nobs) (the
    feedback adds about |go| / 2 to a column); G, G_u, G_obs, OBS ~ N(0,1), mean ~ 0.1 N(0,1), scale ~ U(0.5, 1.5).  W per environment.  The parent
    columns of origin joints in M are NaN.  Made once per case, in the handle's dtype (M: always fp64)."""
    key = (name, dtype, H, B, seed)
    if key not in _inputs:
        s = _spec(name); nx, nu, nobs = s.nx, s.nu, 2 * s.nu
        act_off, na = ACT[name]
        rng = np.random.default_rng(seed); dt = np.float32 if dtype == "f32" else np.float64
        M = rng.standard_normal((H + 1, B, nobs, 24)) / np.sqrt(nobs)
        M[:, :, origin_rows(s), 0:12] = np.nan
        _inputs[key] = dict(
            DZ=(1.3 * rng.standard_normal((H, B, nx, nx)) / np.sqrt(nx)).astype(dt), DU=(rng.standard_normal((H, B, nu, nx)) / np.sqrt(nx)).astype(dt),
            OBS=rng.standard_normal((H + 1, B, nobs)).astype(dt), M=M, W=(rng.standard_normal((B, na, nobs)) / np.sqrt(na)).astype(dt),
            mean=(0.1 * rng.standard_normal(nobs)).astype(dt), scale=rng.uniform(0.5, 1.5, nobs).astype(dt), G=rng.standard_normal((H, B, nx)).astype(dt),
            G_u=rng.standard_normal((H, B, nu)).astype(dt), G_obs=rng.standard_normal((H + 1, B, nobs)).astype(dt))
    return _inputs[key]


CASES = [(m, hb) for m in ("pendulum", "cartpole", "ant") for hb in ((1, 1), (2, 3), (7, 65))] + [("atlas", (3, 5))]


@pytest.mark.parametrize("per_env", [1, 0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,hb", CASES)
def test_sweep_is_the_recursion(name, hb, dtype, per_env):
    """1. synthetic record, no solver involved: nx = 12 (one joint, on the origin; fewer rows than a DPP row), 24, 156 (a body with many child joints),
    372 (more columns than lanes, more observations than a wavefront, 2190 accumulators).  per_env = 0 takes environment 0's W for all and sums
    over the batch (65: not a power of two).  Every output finite: the NaN parent columns of origin joints are never read."""
    H, B = hb
    gm = _handle(name, dtype, B)
    act_off, na = ACT[name]
    inp = dict(synthetic(name, dtype, H, B))
    if not per_env:
        inp["W"] = np.ascontiguousarray(inp["W"][0])
    out = sweep(gm, H, inp, per_env, act_off, na)
    check_all(gm.spec, out, inp, act_off, na, H, dtype == "f32", per_env=bool(per_env))


def test_failed_steps():
    """2. status[2,1] = 1 and NaN Jacobians there: every output finite, environment 1 is the recursion with the cut, gU[2,1] is the control cotangent
    alone, the others do not notice; an all-zero status is no status"""
    H, B = 5, 4
    gm = _handle("ant", "f64", B); act_off, na = ACT["ant"]
    inp = dict(synthetic("ant", "f64", H, B, seed=3))
    clean = sweep(gm, H, inp, 1, act_off, na)
    bad = dict(inp); bad["DZ"] = inp["DZ"].copy(); bad["DU"] = inp["DU"].copy()
    bad["DZ"][2, 1] = np.nan; bad["DU"][2, 1] = np.nan
    status = np.zeros((H, B), np.int32); status[2, 1] = 1
    bad["status"] = status
    out = sweep(gm, H, bad, 1, act_off, na)
    for k in OUTS:
        assert np.isfinite(out[k]).all(), k
    check_all(gm.spec, out, bad, act_off, na, H, False)
    assert np.array_equal(out["gU"][2, 1], inp["G_u"][2, 1])
    for b in (0, 2, 3):
        for k in ("gW", "gbias", "gz"):
            assert same(out[k][b], clean[k][b]), (k, b)
        assert same(out["gU"][:, b], clean["gU"][:, b]), b
    zero = dict(inp); zero["status"] = np.zeros((H, B), np.int32)
    outz = sweep(gm, H, zero, 1, act_off, na)
    for k in OUTS:
        assert same(outz[k], clean[k]), k


def test_deterministic_and_independent_of_the_batch():
    """3. fixed summation order: two runs agree bit for bit, and so does an environment run alone (B = 1) with its place in a batch of 65"""
    H, B = 7, 65
    act_off, na = ACT["ant"]
    inp = synthetic("ant", "f64", H, B)
    gm = _handle("ant", "f64", B)
    o1, o2 = sweep(gm, H, inp, 1, act_off, na), sweep(gm, H, inp, 1, act_off, na)
    for k in OUTS:
        assert same(o1[k], o2[k]), k
    g1 = _handle("ant", "f64", 1)
    for b in (0, 32, 64):
        one = {k: (v if k in ("mean", "scale") else (v[b:b + 1] if k == "W" else v[:, b:b + 1])) for k, v in inp.items()}
        o = sweep(g1, H, one, 1, act_off, na)
        assert same(o["gW"][0], o1["gW"][b]) and same(o["gbias"][0], o1["gbias"][b]) and same(o["gz"][0], o1["gz"][b]) and same(o["gU"][:, 0], o1["gU"][:, b]), b


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_zero_policy_is_the_open_loop_sweep(dtype):
    """4. W = 0, no G_u, no G_obs: gU and gz are dojo_rollout_adjoint_dev's on the same record, within the bound of test 1"""
    H, B = 7, 65
    gm = _handle("ant", dtype, B); s = gm.spec; act_off, na = ACT["ant"]
    inp = dict(synthetic("ant", dtype, H, B)); inp["W"] = np.zeros_like(inp["W"]); inp["G_u"] = None; inp["G_obs"] = None
    out = sweep(gm, H, inp, 1, act_off, na)
    gU = torch.full((H, B, s.nu), float("nan"), dtype=tdt_of(gm), device="cuda"); gz = torch.full((B, s.nx), float("nan"), dtype=tdt_of(gm), device="cuda")
    keep = [dev(inp[k]) for k in ("DZ", "DU", "G")]
    api._chk(api.lib().dojo_rollout_adjoint_dev(gm.h, H, api.addr(keep[0]), api.addr(keep[1]), api.addr(keep[2]), 0, None, None, api.addr(gU), api.addr(gz), api.torch_stream()))
    torch.cuda.synchronize()
    abs_ = recursion(s, absolute(inp), act_off, na, absolute=True)
    n_step = s.nx + 2 * s.nu + na + 8
    check(out["gU"], gU.cpu().numpy().astype(np.float64), abs_["gU"], H, n_step, dtype == "f32", what="gU")
    check(out["gz"], gz.cpu().numpy().astype(np.float64), abs_["gz"], H, n_step, dtype == "f32", what="gz")


def observation_jacobian_dev(gm, z):
    """dojo_observation_jacobian_dev on z [n,B,13Nb] -> compact [n,B,2nu,24]; starts as NaN"""
    n = z.shape[0]
    zd = dev(np.asarray(z, gm.np_dtype))
    M = torch.full((n, gm.batch, 2 * gm.spec.nu, 24), float("nan"), dtype=torch.float64, device="cuda")
    api._chk(api.lib().dojo_observation_jacobian_dev(gm.h, api.addr(zd), n, api.addr(M), api.torch_stream()))
    torch.cuda.synchronize()
    return M.cpu().numpy()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["cartpole", "ant", "atlas"])
def test_observation_jacobian_against_the_oracle(name, dtype):
    """5. densified, against central differences (h = 1e-6) of the oracle's maximal_to_minimal in the attitude convention of tests/fd_coords.py, at z
    (f64) or at the state an fp32 buffer stands for.  Tolerance 1e-6 max(1, max |J|): the finite differences at h = 1e-6 and 2e-6 differ by at
    most 1.7e-8 on these inputs (max |J| <= 5.5), a margin of 60 over the reference's own noise; a wrong sign, factor or column is O(0.1)."""
    from oracle import Oracle
    from fd_coords import fd_coordinate_jacobians
    spec = _spec(name)
    z = d.synthetic_inputs(spec, 3)[0][:2]
    gm = _handle(name, dtype, 2)
    Mc = observation_jacobian_dev(gm, z[None])[0]
    assert np.isfinite(Mc).all()
    assert (Mc[:, origin_rows(spec), 0:12] == 0.0).all()
    assert same(Mc, gm.observation_jacobian(z))                      # the host entry is the same kernel
    J = coords.dense_observation_jacobian(spec, Mc)
    o = Oracle(spec)
    zr = z if dtype == "f64" else d.fp32_abi_state(z)
    for b in range(2):
        JM = fd_coordinate_jacobians(o, o.maximal_to_minimal(zr[b]), zr[b], h=1e-6)[1]
        err = np.abs(J[b] - JM).max()
        print("%s %s env %d: max |J - fd| = %.3e, max |J| = %.3e" % (name, dtype, b, err, np.abs(JM).max()))
        assert err <= 1e-6 * max(1.0, np.abs(JM).max()), (b, err)


_records = {}


def ant_record(B, H=4):
    """Ant f64, contact_forces = 0, through dojo_rollout_policy_dev, dojo_rollout_policy_record_dev and dojo_rollout_record_dev fed with the returned
    U_out; once per batch size (200: two environment groups, spans 128 and 72)"""
    if B not in _records:
        gm = _handle("ant", "f64", B); s = gm.spec; act_off, na = ACT["ant"]; nobs = 2 * s.nu
        if B == 200:
            gm.set_groups(2)
        rng = np.random.default_rng(11)
        p = dict(z0=d.synthetic_inputs(s, B)[0], W=0.1 * rng.standard_normal((B, na, nobs)), bias=0.1 * rng.standard_normal((B, na)),
                 mean=0.1 * rng.standard_normal(nobs), scale=rng.uniform(0.5, 1.5, nobs), U_ff=np.zeros((H, B, s.nu)))
        p["U_ff"][:, :, act_off:act_off + na] = 0.2 * rng.standard_normal((H, B, na))
        t = {k: dev(v) for k, v in p.items()}
        pol = api.DojoPolicy(*[t[k].data_ptr() for k in ("W", "bias", "mean", "scale", "U_ff")], 1, act_off, na, 0, 0, 0)
        f = lambda shape, dt=torch.float64: torch.full(shape, float("nan") if dt == torch.float64 else -123456, dtype=dt, device="cuda")
        L = api.lib()
        a = dict(Z=f((H, B, s.nz)), OBS=f((H + 1, B, nobs)), U=f((H, B, s.nu)), S=f((H, B), torch.int32))
        api._chk(L.dojo_rollout_policy_dev(gm.h, api.addr(t["z0"]), C.byref(pol), H, api.addr(a["Z"]), api.addr(a["OBS"]), api.addr(a["U"]), api.addr(a["S"]), api.torch_stream()))
        r = dict(Z=f((H, B, s.nz)), OBS=f((H + 1, B, nobs)), U=f((H, B, s.nu)), S=f((H, B), torch.int32), DZ=f((H, B, s.nx, s.nx)), DU=f((H, B, s.nu, s.nx)))
        api._chk(L.dojo_rollout_policy_record_dev(gm.h, api.addr(t["z0"]), C.byref(pol), H, api.addr(r["Z"]), api.addr(r["OBS"]), api.addr(r["U"]), api.addr(r["S"]),
                                                  api.addr(r["DZ"]), api.addr(r["DU"]), api.torch_stream()))
        o = dict(Z=f((H, B, s.nz)), S=f((H, B), torch.int32), DZ=f((H, B, s.nx, s.nx)), DU=f((H, B, s.nu, s.nx)))
        api._chk(L.dojo_rollout_record_dev(gm.h, api.addr(t["z0"]), api.addr(r["U"]), H, api.addr(o["Z"]), api.addr(o["S"]), api.addr(o["DZ"]), api.addr(o["DU"]), api.torch_stream()))
        torch.cuda.synchronize()
        _records[B] = (p, {k: v.cpu().numpy() for k, v in a.items()}, {k: v.cpu().numpy() for k, v in r.items()}, {k: v.cpu().numpy() for k, v in o.items()})
    return _records[B]


@pytest.mark.parametrize("B", [64, 200])
def test_record_is_the_two_existing_paths(B):
    """6. Z, OBS, U_out, status bit for bit those of dojo_rollout_policy_dev; DZ, DU on solved steps bit for bit those of dojo_rollout_record_dev fed
    with the returned U_out"""
    p, a, r, o = ant_record(B)
    for k in ("Z", "OBS", "U", "S"):
        assert same(r[k], a[k]), k
    assert same(o["Z"], r["Z"]) and same(o["S"], r["S"])
    ok = r["S"] == 0
    assert ok.mean() >= 0.9
    assert np.isfinite(r["DZ"][ok]).all() and np.isfinite(r["DU"][ok]).all()
    assert same(r["DZ"][ok], o["DZ"][ok]) and same(r["DU"][ok], o["DU"][ok])


def ant_cotangents(B, H=4, seed=9):
    s = _spec("ant"); rng = np.random.default_rng(seed)
    return dict(G=rng.standard_normal((H, B, s.nx)), G_u=rng.standard_normal((H, B, s.nu)), G_obs=rng.standard_normal((H + 1, B, 2 * s.nu)))


def test_null_M_is_the_explicit_M():
    """7. on the record of test 6: the sweep that computes M itself gives the bytes of the sweep given dojo_observation_jacobian_dev([z0; Z])"""
    B, H = 64, 4
    p, _, r, _ = ant_record(B)
    gm = _handle("ant", "f64", B); act_off, na = ACT["ant"]
    M = observation_jacobian_dev(gm, np.concatenate([p["z0"][None], r["Z"]]))
    base = dict(DZ=r["DZ"], DU=r["DU"], OBS=r["OBS"], status=r["S"], W=p["W"], mean=p["mean"], scale=p["scale"], **ant_cotangents(B))
    explicit = sweep(gm, H, dict(base, M=M), 1, act_off, na)
    computed = sweep(gm, H, dict(base, z0=p["z0"], Z=r["Z"]), 1, act_off, na)
    for k in OUTS:
        assert np.isfinite(explicit[k]).all() and same(explicit[k], computed[k]), k


def test_host_entry_end_to_end():
    """8. rollout_policy_gradients on real Jacobians against the recursion over the record of test 6's path and the M of the Jacobian entry"""
    B, H = 64, 4
    p, _, r, _ = ant_record(B)
    gm = _handle("ant", "f64", B); act_off, na = ACT["ant"]
    cot = ant_cotangents(B)
    Z, OBS, U, st, gW, gb, gU, gz = gm.rollout_policy_gradients(p["z0"], p["W"], cot["G"], bias=p["bias"], mean=p["mean"], scale=p["scale"], U_ff=p["U_ff"],
                                                                 act_off=act_off, G_u=cot["G_u"], G_obs=cot["G_obs"])
    assert same(Z, r["Z"]) and same(OBS, r["OBS"]) and same(U, r["U"]) and same(st, r["S"])
    M = observation_jacobian_dev(gm, np.concatenate([p["z0"][None], r["Z"]]))
    inp = dict(DZ=r["DZ"], DU=r["DU"], OBS=r["OBS"], M=M, status=r["S"], W=p["W"], mean=p["mean"], scale=p["scale"], **cot)
    check_all(gm.spec, dict(gW=gW, gbias=gb, gU=gU, gz=gz), inp, act_off, na, H, False)
    assert np.abs(gW).max() > 0


def closed_loop_case(name, B=8, H=6, seed=21):
    """the inputs of tests 9 and 10: z0 of d.synthetic_inputs; cartpole W = -K_REFERENCE uniform(0.5, 1) per environment, pendulum W = 0.1 N(0,1);
    bias = 0.1 N, mean = 0.1 N, scale ~ U(0.5, 1.5), U_ff = 0.2 N on the driven inputs; a loss linear in the x, v, omega components of every Z[k]
    (quaternion columns zero), in U_out and in OBS"""
    spec = _spec(name); act_off, na = ACT[name]; nobs = 2 * spec.nu
    rng = np.random.default_rng(seed)
    z0 = d.synthetic_inputs(spec, B)[0]
    if name == "cartpole":
        W = -K_REFERENCE[None, None, :] * rng.uniform(0.5, 1.0, (B, 1, 1))
    else:
        W = 0.1 * rng.standard_normal((B, na, nobs))
    kw = dict(bias=0.1 * rng.standard_normal((B, na)), mean=0.1 * rng.standard_normal(nobs), scale=rng.uniform(0.5, 1.5, nobs), U_ff=np.zeros((H, B, spec.nu)))
    kw["U_ff"][:, :, act_off:act_off + na] = 0.2 * rng.standard_normal((H, B, na))
    A = rng.standard_normal((H, B, spec.Nb, 13)); A[..., 6:10] = 0.0; A = A.reshape(H, B, spec.nz)
    Bc = rng.standard_normal((H, B, spec.nu)); Cc = rng.standard_normal((H + 1, B, nobs))
    return spec, z0, W, kw, (A, Bc, Cc), rng


def fd_policy_chain_error(name, B=8, H=6, ndir=4, eps=1e-6):
    """-> (worst |fd - an| / max(1, |an|) over the counted environments and directions, fraction of environments counted): <gW, D> + <gbias, Db>
    against central differences of the existing closed-loop rollout"""
    spec, z0, W, kw, (A, Bc, Cc), rng = closed_loop_case(name, B, H)
    act_off, na = ACT[name]
    gm = _handle(name, "f64", B, tight=True)
    _, _, _, st0, gW, gb, _, _ = gm.rollout_policy_gradients(z0, W, A, act_off=act_off, G_u=Bc, G_obs=Cc, cot_space="state", **kw)

    def loss(Wd, bd):
        k2 = dict(kw); k2["bias"] = bd
        Z, OBS, U, st = gm.rollout_policy(z0, Wd, H, act_off=act_off, **k2)
        return (A * Z).sum(axis=(0, 2)) + (Bc * U).sum(axis=(0, 2)) + (Cc * OBS).sum(axis=(0, 2)), st
    worst, counted = 0.0, np.ones(B, bool)
    for _ in range(ndir):
        D = rng.standard_normal(W.shape); Db = rng.standard_normal(kw["bias"].shape)
        Lp, sp = loss(W + eps * D, kw["bias"] + eps * Db); Lm, sm = loss(W - eps * D, kw["bias"] - eps * Db)
        ok = (st0 == 0).all(0) & (sp == 0).all(0) & (sm == 0).all(0)
        counted &= ok
        fd = ((Lp - Lm) / (2 * eps))[ok]
        an = ((gW * D).sum(axis=(1, 2)) + (gb * Db).sum(axis=1))[ok]
        if ok.any():
            worst = max(worst, float((np.abs(fd - an) / np.maximum(1.0, np.abs(an))).max()))
    return worst, counted.mean()


@pytest.mark.parametrize("name", ["cartpole", "pendulum"])
def test_chain_is_the_derivative_of_the_closed_loop(name):
    """9. GRAD_CONSISTENT, rtol = btol = 1e-9, H = 6, B = 8, one policy per environment: the chain against central differences (eps 1e-6) along 4
    random directions in (W, bias).  1e-5 is the project's bound for the open-loop chain at the same eps and tolerances; the CPU oracle alone gives
    2.2e-7 (cartpole) and 1.4e-7 (pendulum) on this experiment."""
    worst, frac = fd_policy_chain_error(name)
    print("%s: worst |fd - an| / max(1, |an|) = %.3e over %.0f %% of the environments" % (name, worst, 100 * frac))
    assert frac >= 0.9
    assert worst <= 1e-5
    if name == "cartpole":
        w_ant, f_ant = fd_policy_chain_error("ant")
        print("ant (contacts, not asserted): worst %.3e over %.0f %% of the environments" % (w_ant, 100 * f_ant))


def test_shared_policy_is_the_sum_over_the_batch():
    """10. test 9's cartpole with one W for all: gW, gbias of per_env = 0 are the sums over b of the per-environment result for the same W tiled,
    within the bound of test 1 with n_red = B (abs_ from the recursion on the downloaded record)"""
    B, H = 8, 6
    spec, z0, W, kw, (A, Bc, Cc), _ = closed_loop_case("cartpole", B, H)
    act_off, na = ACT["cartpole"]
    gm = _handle("cartpole", "f64", B, tight=True)
    W1 = -0.75 * K_REFERENCE[None, :]; b1 = kw["bias"][0]
    k1 = dict(kw, bias=b1); kB = dict(kw, bias=np.tile(b1, (B, 1)))
    sh = gm.rollout_policy_gradients(z0, W1, A, act_off=act_off, G_u=Bc, G_obs=Cc, cot_space="state", **k1)
    pe = gm.rollout_policy_gradients(z0, np.tile(W1, (B, 1, 1)), A, act_off=act_off, G_u=Bc, G_obs=Cc, cot_space="state", **kB)
    for i in range(4):
        assert same(sh[i], pe[i]), i                              # the same rollout
    assert same(sh[6], pe[6]) and same(sh[7], pe[7])              # gU, gz do not depend on how W is given
    assert sh[4].shape == (na, 2 * spec.nu) and sh[5].shape == (na,)
    # abs_: the recursion on the magnitudes of the record the sweep saw
    Z, OBS, st = pe[0], pe[1], pe[3]
    t = {k: dev(v) for k, v in dict(z0=z0, W=np.tile(W1, (B, 1, 1)), bias=kB["bias"], mean=kw["mean"], scale=kw["scale"], U_ff=kw["U_ff"]).items()}
    pol = api.DojoPolicy(*[t[k].data_ptr() for k in ("W", "bias", "mean", "scale", "U_ff")], 1, act_off, na, 0, 0, 0)
    f = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device="cuda")
    r = dict(Z=f((H, B, spec.nz)), OBS=f((H + 1, B, 2 * spec.nu)), U=f((H, B, spec.nu)), S=f((H, B), torch.int32), DZ=f((H, B, spec.nx, spec.nx)), DU=f((H, B, spec.nu, spec.nx)))
    api._chk(api.lib().dojo_rollout_policy_record_dev(gm.h, api.addr(t["z0"]), C.byref(pol), H, api.addr(r["Z"]), api.addr(r["OBS"]), api.addr(r["U"]), api.addr(r["S"]),
                                                      api.addr(r["DZ"]), api.addr(r["DU"]), api.torch_stream()))
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in r.items()}
    assert same(r["Z"], Z) and (r["S"] == 0).all()
    M = observation_jacobian_dev(gm, np.concatenate([z0[None], Z]))
    # (the state-space cotangent in tangent coordinates: x, v, omega are copied; A's quaternion columns are zero, and so is their pull-back g_phi)
    Gt = A.reshape(H, B, spec.Nb, 13)[..., [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12]].reshape(H, B, spec.nx)
    abs_ = recursion(spec, absolute(dict(DZ=r["DZ"], DU=r["DU"], OBS=OBS, M=M, W=W1, mean=kw["mean"], scale=kw["scale"], G=Gt, G_u=Bc, G_obs=Cc)), act_off, na, absolute=True)
    n_step = spec.nx + 2 * spec.nu + na + 8 + 10
    check(sh[4], pe[4].sum(0), abs_["gW"].sum(0), H, n_step, False, n_red=B, what="gW")
    check(sh[5], pe[5].sum(0), abs_["gbias"].sum(0), H, n_step, False, n_red=B, what="gbias")
    assert np.abs(sh[4]).max() > 0


def lift(gz, z0, f32):
    """[B,nx] tangent -> [B,13Nb] state at z0 with dojo_amd.quat: g_q = q0 (x) (0, g_phi)"""
    from dojo_amd import quat
    B = gz.shape[0]
    g = np.asarray(gz, np.float64).reshape(-1, 12); z = np.asarray(z0, np.float64).reshape(-1, 13)
    q = z[:, 6:10].T.copy()
    if f32:
        q = q / np.linalg.norm(q, axis=0)
    gq = quat.qmul(q, np.concatenate([np.zeros((1, g.shape[0])), g[:, 6:9].T])).T
    return np.concatenate([g[:, 0:6], gq, g[:, 9:12]], 1).reshape(B, -1)


def test_autograd_wrapper():
    """11. torch.autograd through differentiable_policy_rollout: the W, bias and U_ff gradients are the host entry's gW, gbias, gU bit for bit (same
    kernels, same buffers' contents), the z0 gradient its gz lifted to state shape, equal to within one unit in the last place of each entry"""
    from dojo_amd.autograd import differentiable_policy_rollout
    B, H = 16, 5
    spec, z0, W, kw, (A, Bc, Cc), _ = closed_loop_case("cartpole", B, H, seed=13)
    act_off, na = ACT["cartpole"]
    f = lambda a: np.asarray(a, np.float32)
    z0, W, A, Bc, Cc = f(z0), f(W), f(A), f(Bc), f(Cc); kw = {k: f(v) for k, v in kw.items()}
    gm = _handle("cartpole", "f32", B)
    Zh, Oh, Uh, sh, gW, gb, gU, gz = gm.rollout_policy_gradients(z0, W, A, act_off=act_off, G_u=Bc, G_obs=Cc, cot_space="state", **kw)
    zt, Wt, bt, Ut = (dev(a).requires_grad_(True) for a in (z0, W, kw["bias"], kw["U_ff"]))
    Z, OBS, U = differentiable_policy_rollout(gm, zt, Wt, bias=bt, U_ff=Ut, mean=dev(kw["mean"]), scale=dev(kw["scale"]), act_off=act_off)
    assert Z.status.dtype == torch.int32 and not Z.status.requires_grad
    loss = (Z * dev(A)).sum() + (U * dev(Bc)).sum() + (OBS * dev(Cc)).sum()
    gzt, gWt, gbt, gUt = torch.autograd.grad(loss, [zt, Wt, bt, Ut])
    torch.cuda.synchronize()
    assert same(Z.detach().cpu().numpy(), Zh) and same(OBS.detach().cpu().numpy(), Oh) and same(U.detach().cpu().numpy(), Uh) and same(Z.status.cpu().numpy(), sh)
    assert same(gWt.cpu().numpy(), gW) and same(gbt.cpu().numpy(), gb) and same(gUt.cpu().numpy(), gU)
    assert np.abs(gW).max() > 0 and np.abs(gU).max() > 0
    ref = lift(gz, z0, True).astype(np.float32)
    got = gzt.cpu().numpy()
    assert got.dtype == np.float32 and np.abs(ref).max() > 0
    assert np.all(np.abs(got - ref) <= np.spacing(np.abs(ref)))


def test_argument_errors():
    """12. every refusal: the stated code, a message on the handle that names the entry point, nothing launched (the outputs keep their fill)"""
    H, B = 2, 3
    gm = _handle("cartpole", "f64", B); s = gm.spec; act_off, na = ACT["cartpole"]
    who = "dojo_rollout_policy_adjoint_dev"
    t = {k: dev(v) for k, v in synthetic("cartpole", "f64", H, B).items()}
    t["M"] = torch.nan_to_num(t["M"])
    t["Z"] = torch.zeros((H, B, s.nz), dtype=torch.float64, device="cuda"); t["z0"] = torch.zeros((B, s.nz), dtype=torch.float64, device="cuda")
    outs = out_tensors(gm, H, 1, na, fill=77.0)
    t.update(outs)

    def refused(what, code, text=who, H_=H, act=(act_off, na), cot_space=0, contact_forces=0, **kw):
        a = dict(t); a.update(kw)
        rc = sweep_raw(gm, H_, a, 1, act[0], act[1], cot_space, contact_forces)
        torch.cuda.synchronize()
        assert rc == code, (what, rc)
        assert text in gm.last_error() and who in gm.last_error(), (what, gm.last_error())
        for k in OUTS:
            assert (outs[k] == 77.0).all(), (what, k)
    refused("H < 1", INVALID, H_=0)
    refused("DZ NULL", INVALID, DZ=None)
    refused("OBS NULL", INVALID, OBS=None)
    refused("G NULL", INVALID, G=None)
    refused("gU without DU", INVALID, DU=None)
    refused("M NULL without z0", INVALID, M=None, z0=None)
    refused("M NULL without Z", INVALID, M=None, Z=None)
    refused("cot_space 1 without Z", INVALID, cot_space=1, Z=None, G=torch.zeros((H, B, s.nz), dtype=torch.float64, device="cuda"))
    refused("DZ unaligned", INVALID, text="16-byte", H_=1, DZ=t["DZ"].view(-1)[1:])
    refused("DU unaligned", INVALID, text="16-byte", H_=1, DU=t["DU"].view(-1)[1:])
    refused("contact_forces", UNSUPPORTED, text="contact_forces", contact_forces=1)
    refused("act_off + na > nu", INVALID, act=(s.nu, 1))
    # ... and the call that is fine writes every output
    assert sweep_raw(gm, H, t, 1, act_off, na) == 0
    torch.cuda.synchronize()
    for k in OUTS:
        assert torch.isfinite(outs[k]).all() and not (outs[k] == 77.0).any(), k
    # nu = 0: a mechanism without inputs
    g0 = _handle("fixed3", "f64", B); s0 = g0.spec
    z = torch.zeros((H, B, s0.nz), dtype=torch.float64, device="cuda")
    t0 = dict(DZ=torch.zeros((H, B, s0.nx, s0.nx), dtype=torch.float64, device="cuda"), DU=z, OBS=z, G=z, W=z, M=z, gz=torch.full((B, s0.nx), 77.0, dtype=torch.float64, device="cuda"))
    assert sweep_raw(g0, H, t0, 1, 0, 1) == INVALID and who in g0.last_error() and "no inputs" in g0.last_error()
    assert (t0["gz"] == 77.0).all()
    Mz = torch.full((B, 1, 24), 77.0, dtype=torch.float64, device="cuda")
    assert api.lib().dojo_observation_jacobian_dev(g0.h, api.addr(z), 1, api.addr(Mz), api.torch_stream()) == INVALID and "dojo_observation_jacobian_dev" in g0.last_error()
    assert (Mz == 77.0).all()
    # the record entry on a mechanism without gradients
    spec = _spec("sphere_linear")
    gs = api.BatchedMechanism(spec, 4, dtype="f64")
    try:
        nobs = 2 * spec.nu
        f = lambda shape, dt=torch.float64: torch.full(shape, 77, dtype=dt, device="cuda")
        W = torch.zeros((spec.nu, nobs), dtype=torch.float64, device="cuda")
        pol = api.DojoPolicy(W.data_ptr(), None, None, None, None, 0, 0, spec.nu, 0, 0, 0)
        z0 = dev(np.tile(d.initialize(spec), (4, 1)))
        r = dict(Z=f((2, 4, spec.nz)), OBS=f((3, 4, nobs)), U=f((2, 4, spec.nu)), S=f((2, 4), torch.int32), DZ=f((2, 4, spec.nx, spec.nx)), DU=f((2, 4, spec.nu, spec.nx)))
        rc = api.lib().dojo_rollout_policy_record_dev(gs.h, api.addr(z0), C.byref(pol), 2, api.addr(r["Z"]), api.addr(r["OBS"]), api.addr(r["U"]), api.addr(r["S"]), api.addr(r["DZ"]), api.addr(r["DU"]), api.torch_stream())
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED and "dojo_rollout_policy_record_dev" in gs.last_error() and "LinearContact" in gs.last_error(), gs.last_error()
        for k, v in r.items():
            assert (v == 77).all(), k
    finally:
        gs.close()
