"""Closed-loop rollouts with a tanh network policy on the GPU, forward and reverse mode (include/dojo_hip.h `DojoMlpPolicy`, csrc/dojo_mlp.hpp): the
one-layer case against the affine entry points bit for bit, the forward kernel layer by layer from what it recorded, the sweep against the recursion
it implements (NumPy fp64 on the same values), the recording entry against the two existing paths, the chain against finite differences of the closed
loop, the shared policy, the host entry, the torch.autograd wrapper and every refusal.

The recursion, per environment, with h_0 = (OBS[k] - mean) .* scale, h_l = ACT[k] (l = 1 .. L-1), M_k the observation Jacobian at the state step k starts from:
    lambda <- g_{H-1} + M_H^T GO_H
    for k = H-1 .. 0:  failed step: lambda <- 0
                       gu = DU_k^T lambda + GU_k -> gU[k];  delta_L = gu[act_off : act_off + na]
                       for l = L .. 1:  g b_l += delta_l;  g W_l += delta_l h_{l-1}^T;  delta_{l-1} = (W_l^T delta_l) .* (1 - h_{l-1}^2)   (no factor for l = 1)
                       go = scale .* delta_0 + GO_k;  lambda = DZ_k^T lambda + M_k^T go (+ g_{k-1} if k > 0)
    gz <- lambda

Error bound of the sweep tests: `check()` of test_policy_adjoint_gpu.py, |out - ref| <= 2 (H n_step + n_red) 2^-53 abs_ (+ 2^-23 |ref| for fp32 outputs), abs_
the same recursion on absolute values with |h_0| <- (|o| + |mean|) |scale| and (1 - h^2) <- (1 + h^2).  The longest chain of one step, recounted in the
kernel's source (rollout_mlp_adjoint_kernel): lambda + g (1), the nx-term column product (nx), delta_L = gu + GU (1), per layer the n_l-term
W_l^T delta_l (n_l) and two more -- fma(-h, h, 1) and its product with the sum, or for l = 1 the scale product and the addition of GO (2) --, the M^T go
sum over the rows that touch a body (at most nobs) and its addition to lambda (1); the accumulators add h_0's subtraction and product and one
multiply-add (3): nx + nobs + sum_l (n_l + 2) + 6.  That is below the count the bound was specified with, n_step = nx + nobs + sum_l (n_l + 3) + 8, which is
the one used.  Ten more where the state cotangent is first pulled back from state coordinates; n_red = B for the output of a shared policy."""
import ctypes as C

import numpy as np
import pytest
import torch

import dojo_amd as d
from dojo_amd import api
from gpu_util import dev, same, tdt_of
import test_policy_adjoint_gpu as P        # the conventions and helpers of the affine tests: same(), synthetic(), check(), absolute(), CASES, ...

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -2
_spec, ACT_OF = P._spec, P.ACT
U53 = 2.0 ** -53

_handles = {}


def _handle(name, dtype, B, tight=False, groups=None):
    """one handle per (mechanism, dtype, batch, options) for the whole module; tight: rtol = btol = 1e-9 and GRAD_CONSISTENT"""
    key = (name, dtype, B, tight, groups)
    if key not in _handles:
        gm = api.BatchedMechanism(_spec(name), B, dtype=dtype, opts=d.SolverOptions(rtol=1e-9, btol=1e-9) if tight else None)
        if tight:
            gm.set_gradient_mode(api.GRAD_CONSISTENT)
        if groups:
            gm.set_groups(groups)
        _handles[key] = gm
    return _handles[key]


def teardown_module(module):
    for gm in _handles.values():
        gm.close()
    _handles.clear()


def widths_of(name, hidden, contact_forces=False):
    s = _spec(name)
    return [2 * s.nu + (len(s.contacts) if contact_forces else 0)] + list(hidden) + [ACT_OF[name][1]]


def random_theta(rng, widths, lead=(), bias=0.1):
    """W_l ~ N(0,1) / sqrt(n_{l-1}), b_l = bias N(0,1), packed"""
    Ws = [rng.standard_normal(lead + (widths[l], widths[l - 1])) / np.sqrt(widths[l - 1]) for l in range(1, len(widths))]
    bs = [bias * rng.standard_normal(lead + (widths[l],)) for l in range(1, len(widths))]
    return api.pack_mlp(Ws, bs)[0]


def hidden_slices(widths):
    o, out = 0, []
    for n in widths[1:-1]:
        out.append(slice(o, o + n)); o += n
    return out


def policy(t, per_env, act_off, widths, contact_forces=0):
    g = lambda k: api.addr(t.get(k))
    return api.mlp_policy_struct(g("theta"), g("mean"), g("scale"), g("U_ff"), per_env, act_off, widths, contact_forces, 0)


def fill(shape, dt):
    return torch.full(shape, float("nan") if dt.is_floating_point else -123456, dtype=dt, device="cuda")


def forward(gm, p, widths, H, per_env, act_off, contact_forces=0, with_act=True, record=False):
    """dojo_rollout_mlp_dev (or the recording entry) on NumPy inputs p (z0, theta, mean, scale, U_ff) -> dict of NumPy outputs; outputs start as NaN"""
    s, B, tdt = gm.spec, gm.batch, tdt_of(gm)
    nobs, nh = widths[0], sum(widths[1:-1])
    t = {k: dev(np.asarray(v, gm.np_dtype)) for k, v in p.items() if v is not None}
    pol = policy(t, per_env, act_off, widths, contact_forces)
    o = dict(Z=fill((H, B, s.nz), tdt), OBS=fill((H + 1, B, nobs), tdt), U=fill((H, B, s.nu), tdt), S=fill((H, B), torch.int32))
    if with_act:
        o["ACT"] = fill((H, B, nh), torch.float64)
    L = api.lib()
    if record:
        o["DZ"] = fill((H, B, s.nx, s.nx), tdt); o["DU"] = fill((H, B, s.nu, s.nx), tdt)
        api._chk(L.dojo_rollout_mlp_record_dev(gm.h, api.addr(t["z0"]), C.byref(pol), H, api.addr(o["Z"]), api.addr(o["OBS"]), api.addr(o["U"]), api.addr(o.get("ACT")), api.addr(o["S"]),
                                               api.addr(o["DZ"]), api.addr(o["DU"]), api.torch_stream()))
    else:
        api._chk(L.dojo_rollout_mlp_dev(gm.h, api.addr(t["z0"]), C.byref(pol), H, api.addr(o["Z"]), api.addr(o["OBS"]), api.addr(o["U"]), api.addr(o.get("ACT")), api.addr(o["S"]), api.torch_stream()))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def closed_loop_inputs(name, dtype, B, H, widths, per_env=1, seed=5, contact_forces=False):
    s = _spec(name); act_off, na = ACT_OF[name]; nobs = widths[0]
    rng = np.random.default_rng(seed); dt = np.float32 if dtype == "f32" else np.float64
    U_ff = np.zeros((H, B, s.nu)); U_ff[:, :, act_off:act_off + na] = 0.2 * rng.standard_normal((H, B, na))
    return dict(z0=d.synthetic_inputs(s, B)[0].astype(dt), theta=random_theta(rng, widths, (B,) if per_env else ()).astype(dt),
                mean=(0.1 * rng.standard_normal(nobs)).astype(dt), scale=rng.uniform(0.5, 1.5, nobs).astype(dt), U_ff=U_ff.astype(dt))


# ---------------------------------------------------------------- 1. one layer is the affine policy, bit for bit ----------------------------------------------------------------
@pytest.mark.parametrize("per_env", [1, 0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,B,cf", [("cartpole", 3, 0), ("ant", 5, 0), ("ant", 5, 1)])
def test_one_layer_forward_is_the_affine_rollout(name, B, cf, dtype, per_env):
    """1a. theta = [W | bias]: Z, OBS, U_out, status of dojo_rollout_mlp_dev are dojo_rollout_policy_dev's (Ant also with its contact observations)"""
    H = 3
    gm = _handle(name, dtype, B); s = gm.spec; act_off, na = ACT_OF[name]; tdt = tdt_of(gm)
    widths = widths_of(name, [], bool(cf)); nobs = widths[0]
    p = closed_loop_inputs(name, dtype, B, H, widths, per_env)
    (W,), (b,) = api.unpack_mlp(p["theta"], widths)
    m = forward(gm, p, widths, H, per_env, act_off, cf)
    t = {k: dev(np.ascontiguousarray(v)) for k, v in dict(p, W=W, bias=b).items()}
    pol = api.DojoPolicy(*[t[k].data_ptr() for k in ("W", "bias", "mean", "scale", "U_ff")], per_env, act_off, na, cf, 0, 0)
    a = dict(Z=fill((H, B, s.nz), tdt), OBS=fill((H + 1, B, nobs), tdt), U=fill((H, B, s.nu), tdt), S=fill((H, B), torch.int32))
    api._chk(api.lib().dojo_rollout_policy_dev(gm.h, api.addr(t["z0"]), C.byref(pol), H, api.addr(a["Z"]), api.addr(a["OBS"]), api.addr(a["U"]), api.addr(a["S"]), api.torch_stream()))
    torch.cuda.synchronize()
    for k in ("Z", "OBS", "U", "S"):
        assert same(m[k], a[k].cpu().numpy()), k
    assert np.nanmax(np.abs(m["U"][:, :, act_off:act_off + na] - p["U_ff"][:, :, act_off:act_off + na])) > 0


def mlp_sweep_raw(gm, H, t, per_env, act_off, widths, cot_space=0, contact_forces=0):
    """dojo_rollout_mlp_adjoint_dev on a dict of torch tensors (missing / None = NULL) -> return code"""
    g = lambda k: api.addr(t.get(k))
    pol = policy(t, per_env, act_off, widths, contact_forces)
    a = api.DojoMlpAdjoint(g("DZ"), g("DU"), g("OBS"), g("ACT"), g("status"), g("z0"), g("Z"), g("M"), g("G"), g("G_u"), g("G_obs"), g("gtheta"), g("gU"), g("gz"),
                           int(cot_space), 0)
    return api.lib().dojo_rollout_mlp_adjoint_dev(gm.h, C.byref(pol), int(H), C.byref(a), api.torch_stream())


OUTS = ("gtheta", "gU", "gz")


def mlp_out_tensors(gm, H, per_env, widths, fill_=float("nan")):
    s, B, tdt = gm.spec, gm.batch, tdt_of(gm)
    Pn = api.mlp_sizes(widths)[0]
    f = lambda shape: torch.full(shape, fill_, dtype=tdt, device="cuda")
    return {"gtheta": f((B, Pn) if per_env else (Pn,)), "gU": f((H, B, s.nu)), "gz": f((B, s.nx))}


def mlp_sweep(gm, H, inp, per_env, act_off, widths, cot_space=0, outs=None):
    """NumPy in, NumPy out (dict over OUTS); the outputs start as NaN so that an entry the kernels leave out shows.
    outs: the caller's own device tensors instead (a missing key = NULL, and missing from the result)"""
    t = {k: dev(v) for k, v in inp.items() if v is not None}
    t.update(mlp_out_tensors(gm, H, per_env, widths) if outs is None else outs)
    api._chk(mlp_sweep_raw(gm, H, t, per_env, act_off, widths, cot_space))
    torch.cuda.synchronize()
    return {k: t[k].cpu().numpy() for k in OUTS if t.get(k) is not None}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["pendulum", "cartpole", "ant"])
@pytest.mark.parametrize("hb", [(1, 1), (2, 3), (7, 65)])
def test_one_layer_sweep_is_the_affine_sweep(name, hb, dtype):
    """1b. synthetic records: gtheta split into [W | b] is gW, gbias of dojo_rollout_policy_adjoint_dev, gU and gz are its gU and gz; per_env 1 and 0"""
    H, B = hb
    gm = _handle(name, dtype, B); act_off, na = ACT_OF[name]
    widths = widths_of(name, [])
    for per_env in (1, 0):
        inp = dict(P.synthetic(name, dtype, H, B))
        if not per_env:
            inp["W"] = np.ascontiguousarray(inp["W"][0])
        aff = P.sweep(gm, H, inp, per_env, act_off, na)
        mi = {k: v for k, v in inp.items() if k != "W"}
        mi["theta"] = api.pack_mlp([inp["W"]], [np.zeros(inp["W"].shape[:-1], inp["W"].dtype)])[0]
        out = mlp_sweep(gm, H, mi, per_env, act_off, widths)
        (gW,), (gb,) = api.unpack_mlp(out["gtheta"], widths)
        assert np.isfinite(out["gtheta"]).all()
        assert same(np.ascontiguousarray(gW), aff["gW"]) and same(np.ascontiguousarray(gb), aff["gbias"]), per_env
        assert same(out["gU"], aff["gU"]) and same(out["gz"], aff["gz"]), per_env


# ---------------------------------------------------------------- 2. forward, layer by layer from what was recorded ----------------------------------------------------------------
FORWARD_CASES = [("pendulum", [3]), ("cartpole", [17, 5]), ("ant", [70]), ("ant", [64, 64, 16])]


def check_layers(p, out, widths, act_off, f32, envs):
    """every layer from the recorded input of that layer; envs: the environments that are checked (every step solved)"""
    Ws, bs = api.unpack_mlp(np.asarray(p["theta"], np.float64), widths)
    L = len(widths) - 1
    sl = hidden_slices(widths)
    na = widths[-1]
    OBS, ACTr, U = out["OBS"].astype(np.float64), out["ACT"], out["U"].astype(np.float64)
    H = U.shape[0]
    mean, scale, U_ff = (np.asarray(p[k], np.float64) for k in ("mean", "scale", "U_ff"))
    dot = lambda W, h: np.einsum("bij,bj->bi", W, h)
    for k in range(H):
        h = (OBS[k] - mean) * scale                                     # the order of the kernel: subtract, multiply
        for l in range(1, L + 1):
            pre, mag = bs[l - 1] + dot(Ws[l - 1], h), np.abs(bs[l - 1]) + dot(np.abs(Ws[l - 1]), np.abs(h))
            lim = 2.0 * (widths[l - 1] + 2) * U53 * mag
            if l < L:
                got = ACTr[k][:, sl[l - 1]]
                err = np.abs(got - np.tanh(pre))
                assert np.isfinite(got[envs]).all() and (np.abs(got[envs]) <= 1.0).all()
                assert ((err - (lim + 6.0 * U53))[envs] <= 0.0).all(), "step %d layer %d: max error %.3e" % (k, l, err[envs].max())
                h = got                                                 # the next layer starts from what was recorded
            else:
                ref = U_ff[k][:, act_off:act_off + na] + pre
                err = np.abs(U[k][:, act_off:act_off + na] - ref)
                # the addition of U_ff is one more fp64 operation (2^-53 |ref|); then one rounding to the handle dtype (fp32: half an ulp, 2^-24 |ref|; fp64: none)
                lim = lim + (U53 + (2.0 ** -24 if f32 else 0.0)) * np.abs(ref)
                assert ((err - lim)[envs] <= 0.0).all(), "step %d output: max error %.3e" % (k, err[envs].max())
        rest = np.ones(U.shape[2], bool); rest[act_off:act_off + na] = False
        assert same(out["U"][k][:, rest], np.asarray(p["U_ff"])[k][:, rest])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("B", [1, 5, 200])
@pytest.mark.parametrize("name,hidden", FORWARD_CASES)
def test_forward_layer_by_layer(name, hidden, B, dtype):
    """2. H = 3; widths narrower than a DPP row, with an odd width, wider than a wavefront and with four layers; B = 1, 5 (a workgroup with dead
    wavefronts), 200 (two environment groups).  Hidden layer l: |ACT - tanh(b_l + W_l h_{l-1})| <= 2 (n_{l-1} + 2) 2^-53 (|b_l| + |W_l| |h_{l-1}|) + 6 2^-53
    with h_{l-1} the RECORDED input (two summation orders of an (n + 1)-term sum, then tanh' <= 1, |tanh| <= 1: 5 ulp of the device library plus 1 of
    NumPy's).  Output: the same dot-product term, 2^-53 |ref| for the fp64 addition of U_ff, plus one rounding to the handle dtype (2^-24 |ref| in fp32).  Z is `rollout` fed the returned
    U_out, bit for bit; ACT = NULL changes nothing."""
    H = 3
    gm = _handle(name, dtype, B, groups=2 if B == 200 else None); s = gm.spec; act_off, na = ACT_OF[name]; tdt = tdt_of(gm)
    widths = widths_of(name, hidden)
    p = closed_loop_inputs(name, dtype, B, H, widths)
    out = forward(gm, p, widths, H, 1, act_off)
    envs = (out["S"] == 0).all(0)
    assert envs.mean() >= 0.9
    assert np.isfinite(out["OBS"][:, envs]).all() and np.isfinite(out["U"][:, envs]).all()
    check_layers(p, out, widths, act_off, dtype == "f32", envs)
    Ud = dev(out["U"]); z0 = dev(p["z0"])
    Z2, S2 = fill((H, B, s.nz), tdt), fill((H, B), torch.int32)
    api._chk(api.lib().dojo_rollout_dev(gm.h, api.addr(z0), api.addr(Ud), H, api.addr(Z2), api.addr(S2), api.torch_stream()))
    torch.cuda.synchronize()
    assert same(Z2.cpu().numpy(), out["Z"]) and same(S2.cpu().numpy(), out["S"])
    bare = forward(gm, p, widths, H, 1, act_off, with_act=False)
    for k in ("Z", "OBS", "U", "S"):
        assert same(bare[k], out[k]), k


# ---------------------------------------------------------------- 3. deterministic and position-independent ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_forward_deterministic_and_independent_of_the_batch(dtype):
    """3. Ant [28, 70, 8], B = 5: two runs give the same bits; an environment alone in B = 1 gives the bits of its place in the batch; per_env = 0 gives the
    bits of the same theta given B times"""
    H, B, name = 3, 5, "ant"
    act_off, na = ACT_OF[name]; widths = widths_of(name, [70])
    gm = _handle(name, dtype, B)
    p = closed_loop_inputs(name, dtype, B, H, widths)
    o1, o2 = forward(gm, p, widths, H, 1, act_off), forward(gm, p, widths, H, 1, act_off)
    for k in o1:
        assert same(o1[k], o2[k]), k
    g1 = _handle(name, dtype, 1)
    for b in (0, 3, 4):
        one = dict(z0=p["z0"][b:b + 1], theta=p["theta"][b:b + 1], mean=p["mean"], scale=p["scale"], U_ff=p["U_ff"][:, b:b + 1])
        o = forward(g1, one, widths, H, 1, act_off)
        for k in o:
            assert same(o[k][:, 0], o1[k][:, b]), (k, b)
    th = np.ascontiguousarray(p["theta"][2])
    sh = forward(gm, dict(p, theta=th), widths, H, 0, act_off)
    ti = forward(gm, dict(p, theta=np.tile(th, (B, 1))), widths, H, 1, act_off)
    for k in sh:
        assert same(sh[k], ti[k]), k


# ---------------------------------------------------------------- 4. the sweep is the recursion ----------------------------------------------------------------
def recursion(spec, inp, act_off, widths, absolute=False):
    """the reference: fp64 NumPy on a dict with DZ [H,B,c,r], DU [H,B,c,r], OBS [H+1,B,nobs], ACT [H,B,nh], M compact [H+1,B,nobs,24], theta [B,P] or [P],
    G [H,B,nx] tangent and optional mean, scale, G_u, G_obs, status.  absolute: |h_0| <- (|o| + |mean|) |scale|, (1 - h^2) <- (1 + h^2) (the inputs are then
    absolute values).  -> dict over OUTS, gtheta per environment."""
    from dojo_amd import coords
    f = lambda k: None if inp.get(k) is None else np.asarray(inp[k], np.float64)
    DZ, DU, OBS, G, GU, GO, A = f("DZ"), f("DU"), f("OBS"), f("G"), f("G_u"), f("G_obs"), f("ACT")
    H, B, nx = G.shape
    nobs, L, na = OBS.shape[2], len(widths) - 1, widths[-1]
    theta = f("theta")
    if theta.ndim == 1:
        theta = np.broadcast_to(theta, (B,) + theta.shape)
    Ws, bs = api.unpack_mlp(theta, widths)
    sl = hidden_slices(widths)
    Md = coords.dense_observation_jacobian(spec, f("M").reshape((H + 1) * B, nobs, 24)).reshape(H + 1, B, nobs, nx)
    mean = np.zeros(nobs) if inp.get("mean") is None else f("mean")
    scale = np.ones(nobs) if inp.get("scale") is None else f("scale")
    status = inp.get("status")
    gWs = [np.zeros(W.shape) for W in Ws]; gbs = [np.zeros(b.shape) for b in bs]; gU = np.zeros((H, B, DU.shape[2]))
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
        hs = [(OBS[k] + mean) * scale if absolute else (OBS[k] - mean) * scale] + [A[k][:, s_] for s_ in sl]
        delta = gu[:, act_off:act_off + na]
        for l in range(L, 0, -1):
            gbs[l - 1] += delta; gWs[l - 1] += delta[:, :, None] * hs[l - 1][:, None, :]
            delta = np.einsum("bij,bi->bj", Ws[l - 1], delta)
            if l > 1:
                delta = delta * ((1.0 + hs[l - 1] ** 2) if absolute else (1.0 - hs[l - 1] ** 2))
        go = scale * delta
        if GO is not None:
            go = go + GO[k]
        lam = new + np.einsum("bro,br->bo", Md[k], go)
        if k > 0:
            lam = lam + G[k - 1]
    return {"gtheta": api.pack_mlp(gWs, gbs)[0], "gU": gU, "gz": lam}


def n_step_of(spec, widths, extra=0):
    return spec.nx + widths[0] + sum(n + 3 for n in widths[1:]) + 8 + extra


def check_all(spec, out, inp, act_off, widths, H, f32, per_env=True, extra=0, abs_G=None):
    """every output in `out` against the recursion on inp; abs_G as in test_policy_adjoint_gpu.check_all"""
    ainp = P.absolute(inp) if abs_G is None else dict(P.absolute(inp), G=abs_G)
    ref, abs_ = recursion(spec, inp, act_off, widths), recursion(spec, ainp, act_off, widths, absolute=True)
    n_step = n_step_of(spec, widths, extra)
    B = np.asarray(inp["G"]).shape[1]
    for k in out:
        shared = (not per_env) and k == "gtheta"
        r, a = (ref[k].sum(0), abs_[k].sum(0)) if shared else (ref[k], abs_[k])
        P.check(out[k], r, a, H, n_step, f32, n_red=B if shared else 0, what=k)
    return ref


_mlp_inputs = {}


def mlp_synthetic(name, dtype, H, B, hidden, seed=7):
    """synthetic()'s record and cotangents (its scales), plus ACT ~ U(-0.95, 0.95) and theta with W_l ~ N(0,1) / sqrt(n_{l-1}), one per environment"""
    key = (name, dtype, H, B, tuple(hidden), seed)
    if key not in _mlp_inputs:
        widths = widths_of(name, hidden)
        rng = np.random.default_rng(seed + 100); dt = np.float32 if dtype == "f32" else np.float64
        inp = {k: v for k, v in P.synthetic(name, dtype, H, B, seed).items() if k != "W"}
        inp["ACT"] = rng.uniform(-0.95, 0.95, (H, B, sum(hidden)))
        inp["theta"] = random_theta(rng, widths, (B,)).astype(dt)
        _mlp_inputs[key] = inp
    return _mlp_inputs[key]


HIDDEN = ([3], [17, 5], [300])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,hb", P.CASES)
def test_sweep_is_the_recursion(name, hb, dtype):
    """4. synthetic record, no solver involved, on the shapes of the affine test; hidden widths [3] (narrower than a DPP row), [17, 5] (three layers, odd)
    and [300] (more hidden units than lanes; Ant: 11108 accumulators per environment); per_env = 0 takes environment 0's theta for all and sums over the
    batch.  Every output finite: the NaN parent columns of origin joints are never read."""
    H, B = hb
    gm = _handle(name, dtype, B); act_off, na = ACT_OF[name]
    for hidden in HIDDEN:
        widths = widths_of(name, hidden)
        for per_env in (1, 0):
            inp = dict(mlp_synthetic(name, dtype, H, B, hidden))
            if not per_env:
                inp["theta"] = np.ascontiguousarray(inp["theta"][0])
            out = mlp_sweep(gm, H, inp, per_env, act_off, widths)
            check_all(gm.spec, out, inp, act_off, widths, H, dtype == "f32", per_env=bool(per_env))
            assert np.abs(out["gtheta"]).max() > 0


def test_sweep_failed_step_and_repeatability():
    """4b. status[2,1] = 1 and NaN Jacobians there: every output finite and the recursion with the cut; the other environments do not notice.  Two runs give
    the same bits, and an environment alone in B = 1 gives the bits of its place in the batch."""
    H, B, name, hidden = 5, 4, "ant", [17, 5]
    gm = _handle(name, "f64", B); act_off, na = ACT_OF[name]; widths = widths_of(name, hidden)
    inp = dict(mlp_synthetic(name, "f64", H, B, hidden, seed=3))
    clean, again = mlp_sweep(gm, H, inp, 1, act_off, widths), mlp_sweep(gm, H, inp, 1, act_off, widths)
    for k in OUTS:
        assert same(clean[k], again[k]), k
    bad = dict(inp); bad["DZ"] = inp["DZ"].copy(); bad["DU"] = inp["DU"].copy()
    bad["DZ"][2, 1] = np.nan; bad["DU"][2, 1] = np.nan
    status = np.zeros((H, B), np.int32); status[2, 1] = 1
    bad["status"] = status
    out = mlp_sweep(gm, H, bad, 1, act_off, widths)
    for k in OUTS:
        assert np.isfinite(out[k]).all(), k
    check_all(gm.spec, out, bad, act_off, widths, H, False)
    assert np.array_equal(out["gU"][2, 1], inp["G_u"][2, 1])
    for b in (0, 2, 3):
        assert same(out["gtheta"][b], clean["gtheta"][b]) and same(out["gz"][b], clean["gz"][b]) and same(out["gU"][:, b], clean["gU"][:, b]), b
    g1 = _handle(name, "f64", 1)
    for b in (0, 3):
        one = {k: (v if k in ("mean", "scale") else (v[b:b + 1] if k == "theta" else v[:, b:b + 1])) for k, v in inp.items()}
        o = mlp_sweep(g1, H, one, 1, act_off, widths)
        assert same(o["gtheta"][0], clean["gtheta"][b]) and same(o["gz"][0], clean["gz"][b]) and same(o["gU"][:, 0], clean["gU"][:, b]), b


# ---------------------------------------------------------------- 5. the recording entry is the two existing paths ----------------------------------------------------------------
_records = {}


def ant_record():
    """Ant f64, B = 64, H = 4, widths [28, 64, 64, 8], one policy per environment: dojo_rollout_mlp_dev, dojo_rollout_mlp_record_dev and
    dojo_rollout_record_dev fed with the returned U_out; made once"""
    if "ant" not in _records:
        B, H, name = 64, 4, "ant"
        gm = _handle(name, "f64", B); s = gm.spec; act_off, na = ACT_OF[name]; widths = widths_of(name, [64, 64])
        p = closed_loop_inputs(name, "f64", B, H, widths, seed=11)
        a = forward(gm, p, widths, H, 1, act_off)
        r = forward(gm, p, widths, H, 1, act_off, record=True)
        f = lambda shape, dt=torch.float64: fill(shape, dt)
        o = dict(Z=f((H, B, s.nz)), S=f((H, B), torch.int32), DZ=f((H, B, s.nx, s.nx)), DU=f((H, B, s.nu, s.nx)))
        z0, Ud = dev(p["z0"]), dev(r["U"])
        api._chk(api.lib().dojo_rollout_record_dev(gm.h, api.addr(z0), api.addr(Ud), H, api.addr(o["Z"]), api.addr(o["S"]), api.addr(o["DZ"]), api.addr(o["DU"]), api.torch_stream()))
        torch.cuda.synchronize()
        _records["ant"] = (p, widths, a, r, {k: v.cpu().numpy() for k, v in o.items()})
    return _records["ant"]


def test_record_is_the_two_existing_paths():
    """5. Z, OBS, U_out, ACT, status bit for bit those of dojo_rollout_mlp_dev; DZ, DU on solved steps bit for bit those of dojo_rollout_record_dev fed with
    the returned U_out"""
    p, widths, a, r, o = ant_record()
    for k in ("Z", "OBS", "U", "ACT", "S"):
        assert same(r[k], a[k]), k
    assert np.isfinite(r["ACT"]).all() and np.abs(r["ACT"]).max() > 0
    assert same(o["Z"], r["Z"]) and same(o["S"], r["S"])
    ok = r["S"] == 0
    assert ok.mean() >= 0.9
    assert np.isfinite(r["DZ"][ok]).all() and np.isfinite(r["DU"][ok]).all()
    assert same(r["DZ"][ok], o["DZ"][ok]) and same(r["DU"][ok], o["DU"][ok])


# ---------------------------------------------------------------- 6. the chain is the derivative of the closed loop ----------------------------------------------------------------
def closed_loop_case(name, hidden, B=8, H=6, seed=21, per_env=True):
    """z0 of d.synthetic_inputs; W_l = N(0,1) / sqrt(n_{l-1}), b_l = 0.1 N, mean = 0.1 N, scale ~ U(0.5, 1.5), U_ff = 0.2 N on the driven inputs; a loss linear in
    the x, v, omega components of every Z[k] (quaternion columns zero), in U_out and in OBS"""
    spec = _spec(name); act_off, na = ACT_OF[name]; widths = widths_of(name, hidden); nobs = widths[0]
    rng = np.random.default_rng(seed)
    z0 = d.synthetic_inputs(spec, B)[0]
    theta = random_theta(rng, widths, (B,) if per_env else ())
    kw = dict(mean=0.1 * rng.standard_normal(nobs), scale=rng.uniform(0.5, 1.5, nobs), U_ff=np.zeros((H, B, spec.nu)))
    kw["U_ff"][:, :, act_off:act_off + na] = 0.2 * rng.standard_normal((H, B, na))
    A = rng.standard_normal((H, B, spec.Nb, 13)); A[..., 6:10] = 0.0; A = A.reshape(H, B, spec.nz)
    Bc = rng.standard_normal((H, B, spec.nu)); Cc = rng.standard_normal((H + 1, B, nobs))
    return spec, widths, z0, theta, kw, (A, Bc, Cc), rng


def fd_chain_error(name, hidden, B=8, H=6, ndir=4, eps=1e-6):
    """-> (worst |fd - an| / max(1, |an|) over the counted environments and directions, fraction of environments counted): <gtheta, D> against central
    differences of rollout_mlp"""
    spec, widths, z0, theta, kw, (A, Bc, Cc), rng = closed_loop_case(name, hidden, B, H)
    act_off, na = ACT_OF[name]
    gm = _handle(name, "f64", B, tight=True)
    _, _, _, st0, gth, _, _ = gm.rollout_mlp_gradients(z0, theta, widths, A, act_off=act_off, G_u=Bc, G_obs=Cc, cot_space="state", **kw)

    def loss(th):
        Z, OBS, U, st = gm.rollout_mlp(z0, th, widths, H, act_off=act_off, **kw)
        return (A * Z).sum(axis=(0, 2)) + (Bc * U).sum(axis=(0, 2)) + (Cc * OBS).sum(axis=(0, 2)), st
    worst, counted = 0.0, np.ones(B, bool)
    for _ in range(ndir):
        D = rng.standard_normal(theta.shape)
        Lp, sp = loss(theta + eps * D); Lm, sm = loss(theta - eps * D)
        ok = (st0 == 0).all(0) & (sp == 0).all(0) & (sm == 0).all(0)
        counted &= ok
        fd = ((Lp - Lm) / (2 * eps))[ok]
        an = (gth * D).sum(axis=1)[ok]
        if ok.any():
            worst = max(worst, float((np.abs(fd - an) / np.maximum(1.0, np.abs(an))).max()))
    return worst, counted.mean()


@pytest.mark.parametrize("name,hidden", [("cartpole", [5, 3]), ("pendulum", [17])])
def test_chain_is_the_derivative_of_the_closed_loop(name, hidden):
    """6. GRAD_CONSISTENT, rtol = btol = 1e-9, fp64, H = 6, B = 8, one policy per environment: the chain against central differences (eps 1e-6) of rollout_mlp
    along 4 random directions in theta.  1e-5 is the project's bound for this experiment (the affine and the open-loop chain at the same eps and
    tolerances); the CPU oracle's own chain gives 6.1e-8 (cartpole [4,5,3,1]) and 1.7e-7 (pendulum [2,17,1])."""
    worst, frac = fd_chain_error(name, hidden)
    print("%s %s: worst |fd - an| / max(1, |an|) = %.3e over %.0f %% of the environments" % (name, widths_of(name, hidden), worst, 100 * frac))
    assert frac >= 0.9
    assert worst <= 1e-5


# ---------------------------------------------------------------- 7. shared policy ----------------------------------------------------------------
def test_shared_policy_is_the_sum_over_the_batch():
    """7. test 6's cartpole with one theta for all: gtheta of per_env = 0 is the sum over b of the per-environment result for the same theta tiled, within
    the bound of test 4 with n_red = B (abs_ from the recursion on the downloaded record); the rollout, gU and gz are equal bit for bit"""
    B, H, name, hidden = 8, 6, "cartpole", [5, 3]
    spec, widths, z0, theta, kw, (A, Bc, Cc), _ = closed_loop_case(name, hidden, B, H, per_env=False)
    act_off, na = ACT_OF[name]
    gm = _handle(name, "f64", B, tight=True)
    tiled = np.tile(theta, (B, 1))
    sh = gm.rollout_mlp_gradients(z0, theta, widths, A, act_off=act_off, G_u=Bc, G_obs=Cc, cot_space="state", **kw)
    pe = gm.rollout_mlp_gradients(z0, tiled, widths, A, act_off=act_off, G_u=Bc, G_obs=Cc, cot_space="state", **kw)
    for i in range(4):
        assert same(sh[i], pe[i]), i                              # the same rollout
    assert same(sh[5], pe[5]) and same(sh[6], pe[6])              # gU, gz do not depend on how theta is given
    assert sh[4].shape == theta.shape and pe[4].shape == tiled.shape
    r = forward(gm, dict(z0=z0, theta=tiled, **kw), widths, H, 1, act_off, record=True)
    assert same(r["Z"], pe[0]) and (r["S"] == 0).all()
    M = P.observation_jacobian_dev(gm, np.concatenate([z0[None], pe[0]]))
    # (the state-space cotangent in tangent coordinates: x, v, omega are copied; A's quaternion columns are zero, and so is their pull-back g_phi)
    Gt = A.reshape(H, B, spec.Nb, 13)[..., [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12]].reshape(H, B, spec.nx)
    rec = dict(DZ=r["DZ"], DU=r["DU"], OBS=r["OBS"], ACT=r["ACT"], M=M, theta=theta, mean=kw["mean"], scale=kw["scale"], G=Gt, G_u=Bc, G_obs=Cc)
    abs_ = recursion(spec, P.absolute(rec), act_off, widths, absolute=True)
    P.check(sh[4], pe[4].sum(0), abs_["gtheta"].sum(0), H, n_step_of(spec, widths, 10), False, n_red=B, what="gtheta")
    assert np.abs(sh[4]).max() > 0


# ---------------------------------------------------------------- 8. host entry and autograd ----------------------------------------------------------------
def test_host_entry_end_to_end():
    """8a. rollout_mlp_gradients on real Jacobians against the recursion over the record of test 5 and the M of the Jacobian entry"""
    p, widths, _, r, _ = ant_record()
    B, H = 64, 4
    gm = _handle("ant", "f64", B); act_off, na = ACT_OF["ant"]
    cot = P.ant_cotangents(B)
    Z, OBS, U, st, gth, gU, gz = gm.rollout_mlp_gradients(p["z0"], p["theta"], widths, cot["G"], mean=p["mean"], scale=p["scale"], U_ff=p["U_ff"], act_off=act_off,
                                                          G_u=cot["G_u"], G_obs=cot["G_obs"])
    assert same(Z, r["Z"]) and same(OBS, r["OBS"]) and same(U, r["U"]) and same(st, r["S"])
    M = P.observation_jacobian_dev(gm, np.concatenate([p["z0"][None], r["Z"]]))
    inp = dict(DZ=r["DZ"], DU=r["DU"], OBS=r["OBS"], ACT=r["ACT"], M=M, status=r["S"], theta=p["theta"], mean=p["mean"], scale=p["scale"], **cot)
    check_all(gm.spec, dict(gtheta=gth, gU=gU, gz=gz), inp, act_off, widths, H, False)
    assert np.abs(gth).max() > 0


@pytest.mark.parametrize("per_env", [1, 0])
def test_autograd_wrapper(per_env):
    """8b. cartpole fp32, B = 16, H = 5, widths [4, 5, 3, 1]: torch.autograd through differentiable_mlp_rollout returns the host entry's gtheta and gU bit
    for bit (same kernels, same buffers' contents); the z0 gradient is its gz lifted to state shape, to one unit in the last place"""
    from dojo_amd.autograd import differentiable_mlp_rollout
    B, H, name, hidden = 16, 5, "cartpole", [5, 3]
    spec, widths, z0, theta, kw, (A, Bc, Cc), _ = closed_loop_case(name, hidden, B, H, seed=13, per_env=bool(per_env))
    act_off, na = ACT_OF[name]
    f = lambda a: np.asarray(a, np.float32)
    z0, theta, A, Bc, Cc = f(z0), f(theta), f(A), f(Bc), f(Cc); kw = {k: f(v) for k, v in kw.items()}
    gm = _handle(name, "f32", B)
    Zh, Oh, Uh, sh, gth, gU, gz = gm.rollout_mlp_gradients(z0, theta, widths, A, act_off=act_off, G_u=Bc, G_obs=Cc, cot_space="state", **kw)
    zt, tt, Ut = (dev(a).requires_grad_(True) for a in (z0, theta, kw["U_ff"]))
    Z, OBS, U = differentiable_mlp_rollout(gm, zt, tt, widths, U_ff=Ut, mean=dev(kw["mean"]), scale=dev(kw["scale"]), act_off=act_off)
    assert Z.status.dtype == torch.int32 and not Z.status.requires_grad
    loss = (Z * dev(A)).sum() + (U * dev(Bc)).sum() + (OBS * dev(Cc)).sum()
    gzt, gtt, gUt = torch.autograd.grad(loss, [zt, tt, Ut])
    torch.cuda.synchronize()
    assert same(Z.detach().cpu().numpy(), Zh) and same(OBS.detach().cpu().numpy(), Oh) and same(U.detach().cpu().numpy(), Uh) and same(Z.status.cpu().numpy(), sh)
    assert same(gtt.cpu().numpy(), gth) and same(gUt.cpu().numpy(), gU)
    assert gth.shape == theta.shape and np.abs(gth).max() > 0 and np.abs(gU).max() > 0
    ref = P.lift(gz, z0, True).astype(np.float32)
    got = gzt.cpu().numpy()
    assert got.dtype == np.float32 and np.abs(ref).max() > 0
    assert np.all(np.abs(got - ref) <= np.spacing(np.abs(ref)))


# ---------------------------------------------------------------- 9. refusals ----------------------------------------------------------------
def test_forward_argument_errors():
    """9a. dojo_rollout_mlp_dev and dojo_rollout_mlp_record_dev: the stated code, a message on the handle that names the entry point, nothing launched (the
    outputs keep their fill)"""
    H, B, name = 2, 3, "cartpole"
    gm = _handle(name, "f64", B); s = gm.spec; act_off, na = ACT_OF[name]
    widths = widths_of(name, [5, 3]); nh = 8
    p = closed_loop_inputs(name, "f64", B, H, widths)
    t = {k: dev(v) for k, v in p.items()}
    f = lambda shape, dt=torch.float64: torch.full(shape, 77, dtype=dt, device="cuda")
    o = dict(Z=f((H, B, s.nz)), OBS=f((H + 1, B, 2 * s.nu)), U=f((H, B, s.nu)), ACT=f((H, B, nh)), S=f((H, B), torch.int32), DZ=f((H, B, s.nx, s.nx)), DU=f((H, B, s.nu, s.nx)))
    L = api.lib()

    def call(record, w=widths, act=act_off, H_=H, cf=0, n_layers=None, z0="z0", theta="theta", **null):
        a = {k: (None if null.get(k, 1) is None else v) for k, v in o.items()}
        pol = policy(dict(t, theta=t.get(theta)), 1, act, w, cf)
        if n_layers is not None:
            pol.n_layers = n_layers
        if record:
            return L.dojo_rollout_mlp_record_dev(gm.h, api.addr(t.get(z0)), C.byref(pol), H_, api.addr(a["Z"]), api.addr(a["OBS"]), api.addr(a["U"]), api.addr(a["ACT"]), api.addr(a["S"]),
                                                 api.addr(a["DZ"]), api.addr(a["DU"]), api.torch_stream())
        return L.dojo_rollout_mlp_dev(gm.h, api.addr(t.get(z0)), C.byref(pol), H_, api.addr(a["Z"]), api.addr(a["OBS"]), api.addr(a["U"]), api.addr(a["ACT"]), api.addr(a["S"]), api.torch_stream())

    def refused(what, code, text="", entries=(0, 1), **kw):
        for record in entries:
            who = "dojo_rollout_mlp_record_dev" if record else "dojo_rollout_mlp_dev"
            rc = call(record, **kw)
            torch.cuda.synchronize()
            assert rc == code, (what, who, rc)
            assert who in gm.last_error() and text in gm.last_error(), (what, gm.last_error())
            for k, v in o.items():
                assert (v == 77).all(), (what, who, k)
    refused("z0 NULL", INVALID, z0="none")
    refused("theta NULL", INVALID, theta="none")
    refused("H < 1", INVALID, H_=0)
    refused("n_layers 0", INVALID, text="n_layers", n_layers=0)
    refused("n_layers 5", INVALID, text="n_layers", n_layers=5)
    refused("a width < 1", INVALID, text="width[1]", w=[4, 0, 3, 1])
    refused("width[0] != nobs", INVALID, text="width[0]", w=[5, 5, 3, 1])
    refused("act_off + na > nu", INVALID, act=s.nu)
    refused("act_off < 0", INVALID, act=-1)
    refused("act_off + width[L] > nu", INVALID, w=[4, 5, 3, 3])
    refused("LDS", UNSUPPORTED, text="LDS", w=[4, 9000, 1])
    refused("2^31 parameters or more", UNSUPPORTED, text="2^31", w=[4, 60000, 60000, 1])
    refused("ACT NULL with L > 1", INVALID, text="ACT", entries=(1,), ACT=None)
    refused("DZ NULL", INVALID, entries=(1,), DZ=None)
    refused("U_out NULL", INVALID, entries=(1,), U=None)
    # ... and the calls that are fine write every output (the forward entry with every output NULL is fine too)
    assert call(0) == 0 and call(1) == 0
    torch.cuda.synchronize()
    for k, v in o.items():
        assert not (v == 77).any(), k
    assert call(0, Z=None, OBS=None, U=None, ACT=None, S=None) == 0
    torch.cuda.synchronize()
    # contact_init = 1 on a handle without a solution (a fresh one)
    gf = api.BatchedMechanism(s, B, dtype="f64")
    try:
        pol = policy(t, 1, act_off, widths); pol.contact_init = 1
        rc = L.dojo_rollout_mlp_dev(gf.h, api.addr(t["z0"]), C.byref(pol), H, api.addr(o["Z"]), api.addr(o["OBS"]), api.addr(o["U"]), api.addr(o["ACT"]), api.addr(o["S"]), api.torch_stream())
        torch.cuda.synchronize()
        assert rc == INVALID and "dojo_rollout_mlp_dev" in gf.last_error() and "contact_init" in gf.last_error(), gf.last_error()
    finally:
        gf.close()
    # a mechanism without inputs; a mechanism with a kinematic loop; a mechanism without gradients in the recording entry
    g0 = _handle("fixed3", "f64", B)
    z = torch.zeros((H, B, g0.spec.nz), dtype=torch.float64, device="cuda")
    pol = api.mlp_policy_struct(z.data_ptr(), None, None, None, 1, 0, [1, 1])
    assert L.dojo_rollout_mlp_dev(g0.h, api.addr(z), C.byref(pol), H, None, None, None, None, None, api.torch_stream()) == INVALID
    assert "dojo_rollout_mlp_dev" in g0.last_error() and "no inputs" in g0.last_error()
    gl = api.BatchedMechanism(d.get_fourbar(), 2, dtype="f64")
    try:
        sl = gl.spec; w = [2 * sl.nu, 3, 1]
        z0l = torch.zeros((2, sl.nz), dtype=torch.float64, device="cuda"); th = torch.zeros(api.mlp_sizes(w)[0], dtype=torch.float64, device="cuda")
        Ul = f((H, 2, sl.nu))
        pol = api.mlp_policy_struct(th.data_ptr(), None, None, None, 0, 0, w)
        rc = L.dojo_rollout_mlp_dev(gl.h, api.addr(z0l), C.byref(pol), H, None, None, api.addr(Ul), None, None, api.torch_stream())
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED and "dojo_rollout_mlp_dev" in gl.last_error() and "loop" in gl.last_error(), gl.last_error()
        assert (Ul == 77).all()
    finally:
        gl.close()
    spec = _spec("sphere_linear")
    gs = api.BatchedMechanism(spec, 4, dtype="f64")
    try:
        nobs = 2 * spec.nu; w = [nobs, 3, spec.nu]
        th = torch.zeros(api.mlp_sizes(w)[0], dtype=torch.float64, device="cuda")
        pol = api.mlp_policy_struct(th.data_ptr(), None, None, None, 0, 0, w)
        z0 = dev(np.tile(d.initialize(spec), (4, 1)))
        r = dict(Z=f((2, 4, spec.nz)), OBS=f((3, 4, nobs)), U=f((2, 4, spec.nu)), ACT=f((2, 4, 3)), S=f((2, 4), torch.int32), DZ=f((2, 4, spec.nx, spec.nx)), DU=f((2, 4, spec.nu, spec.nx)))
        rc = L.dojo_rollout_mlp_record_dev(gs.h, api.addr(z0), C.byref(pol), 2, api.addr(r["Z"]), api.addr(r["OBS"]), api.addr(r["U"]), api.addr(r["ACT"]), api.addr(r["S"]), api.addr(r["DZ"]), api.addr(r["DU"]), api.torch_stream())
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED and "dojo_rollout_mlp_record_dev" in gs.last_error() and "LinearContact" in gs.last_error(), gs.last_error()
        for k, v in r.items():
            assert (v == 77).all(), k
    finally:
        gs.close()


def test_adjoint_argument_errors():
    """9b. dojo_rollout_mlp_adjoint_dev and the host entry dojo_rollout_mlp_gradients"""
    H, B, name, hidden = 2, 3, "cartpole", [5, 3]
    gm = _handle(name, "f64", B); s = gm.spec; act_off, na = ACT_OF[name]; widths = widths_of(name, hidden)
    who = "dojo_rollout_mlp_adjoint_dev"
    t = {k: dev(v) for k, v in mlp_synthetic(name, "f64", H, B, hidden).items()}
    t["M"] = torch.nan_to_num(t["M"])
    t["Z"] = torch.zeros((H, B, s.nz), dtype=torch.float64, device="cuda"); t["z0"] = torch.zeros((B, s.nz), dtype=torch.float64, device="cuda")
    outs = mlp_out_tensors(gm, H, 1, widths, fill_=77.0)
    t.update(outs)

    def refused(what, code, text=who, H_=H, act=act_off, w=widths, cot_space=0, contact_forces=0, n_layers=None, **kw):
        a = dict(t); a.update(kw)
        if n_layers is None:
            rc = mlp_sweep_raw(gm, H_, a, 1, act, w, cot_space, contact_forces)
        else:
            g = lambda k: api.addr(a.get(k))
            pol = policy(a, 1, act, w, contact_forces); pol.n_layers = n_layers
            ad = api.DojoMlpAdjoint(g("DZ"), g("DU"), g("OBS"), g("ACT"), g("status"), g("z0"), g("Z"), g("M"), g("G"), g("G_u"), g("G_obs"), g("gtheta"), g("gU"), g("gz"), 0, 0)
            rc = api.lib().dojo_rollout_mlp_adjoint_dev(gm.h, C.byref(pol), H_, C.byref(ad), api.torch_stream())
        torch.cuda.synchronize()
        assert rc == code, (what, rc)
        assert text in gm.last_error() and who in gm.last_error(), (what, gm.last_error())
        for k in OUTS:
            assert (outs[k] == 77.0).all(), (what, k)
    refused("H < 1", INVALID, H_=0)
    refused("theta NULL", INVALID, theta=None)
    refused("DZ NULL", INVALID, DZ=None)
    refused("OBS NULL", INVALID, OBS=None)
    refused("G NULL", INVALID, G=None)
    refused("without DU", INVALID, DU=None)
    refused("ACT NULL with L > 1", INVALID, text="ACT", ACT=None)
    refused("M NULL without z0", INVALID, M=None, z0=None)
    refused("M NULL without Z", INVALID, M=None, Z=None)
    refused("cot_space 1 without Z", INVALID, cot_space=1, Z=None, G=torch.zeros((H, B, s.nz), dtype=torch.float64, device="cuda"))
    refused("DZ unaligned", INVALID, text="16-byte", H_=1, DZ=t["DZ"].view(-1)[1:])
    refused("DU unaligned", INVALID, text="16-byte", H_=1, DU=t["DU"].view(-1)[1:])
    refused("contact_forces", UNSUPPORTED, text="contact_forces", contact_forces=1)
    refused("act_off + na > nu", INVALID, act=s.nu)
    refused("act_off < 0", INVALID, act=-1)
    refused("n_layers 0", INVALID, text="n_layers", n_layers=0)
    refused("n_layers 5", INVALID, text="n_layers", n_layers=5)
    refused("a width < 1", INVALID, text="width[2]", w=[4, 5, 0, 1])
    refused("width[0] != nobs", INVALID, text="width[0]", w=[3, 5, 3, 1])
    refused("LDS", UNSUPPORTED, text="4 (nobs + nh)", w=[4, 9000, 1])       # (the forward kernel's need; the sweep's own: test_sweep_lds_limit below)
    refused("2^31 parameters or more", UNSUPPORTED, text="2^31", w=[4, 2 ** 31 - 1, 2 ** 31 - 1, 1])
    # ... and the call that is fine writes every output
    assert mlp_sweep_raw(gm, H, t, 1, act_off, widths) == 0
    torch.cuda.synchronize()
    for k in OUTS:
        assert torch.isfinite(outs[k]).all() and not (outs[k] == 77.0).any(), k
    # the host entry: contact_forces cannot be asked for through the binding, so the struct is built here
    whoh = "dojo_rollout_mlp_gradients"
    z0 = np.zeros((B, s.nz)); th = np.zeros(api.mlp_sizes(widths)[0]); G = np.zeros((H, B, s.nx)); gth = np.full_like(th, 77.0)
    for cf, w, code, text in ((1, widths, UNSUPPORTED, "contact_forces"), (0, [4, 5, 3, 3], INVALID, ""), (0, [4, 9000, 1], UNSUPPORTED, "LDS")):
        pol = api.mlp_policy_struct(th.ctypes.data, None, None, None, 0, act_off, w, cf, 0)
        rc = api.lib().dojo_rollout_mlp_gradients(gm.h, api.addr(z0), C.byref(pol), H, api.addr(G), 0, None, None, None, None, None, None, api.addr(gth), None, None)
        assert rc == code and whoh in gm.last_error() and text in gm.last_error(), (cf, w, rc, gm.last_error())
        assert (gth == 77.0).all()
    with pytest.raises(api.DojoError, match="dojo_rollout_mlp:"):
        gm.rollout_mlp(z0, np.zeros(api.mlp_sizes([3, 5, 3, 1])[0]), [3, 5, 3, 1], H)


# ---------------------------------------------------------------- 9c. the sweep's own LDS limit ----------------------------------------------------------------
SWEEP_LDS = "4 nx + nu + 2 nobs + 2 wmax + nh"


def nslider60_inputs(widths, H, B, seed=17):
    """a 60-body chain of sliders (nx = 720, nu = 60, nobs = 120), synthetic()'s scales, one policy per environment, fp64"""
    spec = d.get_nslider(num_bodies=60); nx, nu, nobs = spec.nx, spec.nu, 2 * spec.nu
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((H + 1, B, nobs, 24)) / np.sqrt(nobs)
    M[:, :, P.origin_rows(spec), 0:12] = np.nan
    return dict(DZ=1.3 * rng.standard_normal((H, B, nx, nx)) / np.sqrt(nx), DU=rng.standard_normal((H, B, nu, nx)) / np.sqrt(nx), OBS=rng.standard_normal((H + 1, B, nobs)), M=M,
                mean=0.1 * rng.standard_normal(nobs), scale=rng.uniform(0.5, 1.5, nobs), G=rng.standard_normal((H, B, nx)), G_u=rng.standard_normal((H, B, nu)),
                G_obs=rng.standard_normal((H + 1, B, nobs)), ACT=rng.uniform(-0.95, 0.95, (H, B, sum(widths[1:-1]))), theta=random_theta(rng, widths, (B,)))


def test_sweep_lds_limit():
    """9c. The sweep keeps 4 nx + nu + 2 nobs + 2 wmax + nh doubles in LDS.  On a 60-body nslider (2880 + 60 + 240 = 3180 before the policy) the widths
    [120, 1700, 1] pass the forward check (4 (120 + 1700) doubles = 58 240 bytes) and need 3180 + 3400 + 1700 = 8280 doubles > 8192 in the sweep: refused by
    dojo_rollout_mlp_adjoint_dev and dojo_rollout_mlp_gradients with DOJO_ERR_UNSUPPORTED and the sweep's own message, outputs untouched.  [120, 1670, 1]
    needs 8190 doubles = 65 520 bytes, 16 below the limit: it runs, and is the recursion within the bound of test 4 -- the formula covers the kernel's
    LDS layout (a layout that needed more would overrun the allocation here)."""
    H, B = 2, 2
    spec = d.get_nslider(num_bodies=60)
    assert (spec.nx, spec.nu) == (720, 60)
    gm = api.BatchedMechanism(spec, B, dtype="f64")
    try:
        big, fits = [120, 1700, 1], [120, 1670, 1]
        assert 4 * (120 + 1700) * 8 <= 65536 < (3180 + 3 * 1700) * 8 and (3180 + 3 * 1670) * 8 <= 65536
        inp = nslider60_inputs(big, H, B)
        t = {k: dev(v) for k, v in inp.items()}
        t["M"] = torch.nan_to_num(t["M"])
        outs = mlp_out_tensors(gm, H, 1, big, fill_=77.0)
        t.update(outs)
        rc = mlp_sweep_raw(gm, H, t, 1, 0, big)
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED and "dojo_rollout_mlp_adjoint_dev" in gm.last_error() and SWEEP_LDS in gm.last_error(), (rc, gm.last_error())
        for k in OUTS:
            assert (outs[k] == 77.0).all(), k
        z0 = np.zeros((B, spec.nz)); th = np.zeros(api.mlp_sizes(big)[0]); G = np.zeros((H, B, spec.nx)); gth = np.full_like(th, 77.0)
        gU = np.full((H, B, spec.nu), 77.0); gz = np.full((B, spec.nx), 77.0)
        pol = api.mlp_policy_struct(th.ctypes.data, None, None, None, 0, 0, big)
        rc = api.lib().dojo_rollout_mlp_gradients(gm.h, api.addr(z0), C.byref(pol), H, api.addr(G), 0, None, None, None, None, None, None, api.addr(gth), api.addr(gU), api.addr(gz))
        assert rc == UNSUPPORTED and "dojo_rollout_mlp_gradients" in gm.last_error() and SWEEP_LDS in gm.last_error(), (rc, gm.last_error())
        assert (gth == 77.0).all() and (gU == 77.0).all() and (gz == 77.0).all()
        del t, outs
        inp = nslider60_inputs(fits, H, B)
        out = mlp_sweep(gm, H, inp, 1, 0, fits)
        check_all(spec, out, inp, 0, fits, H, False)
        assert np.abs(out["gtheta"]).max() > 0
    finally:
        gm.close()
