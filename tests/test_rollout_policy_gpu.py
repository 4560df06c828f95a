"""Closed-loop rollouts on the GPU: dojo_rollout_policy_dev / dojo_rollout_policy, u_k = U_ff[k] + E (bias + W ((o_k - mean) .* scale)) with o_k the
observation of the state step k starts from, evaluated by the library between the steps (csrc/dojo_policy.hpp).

Two closed-loop trajectories of a contact-rich system cannot be compared to a tolerance (they diverge), so the loop is proved link by link, each exact:
  1. the steps consumed U_out:        dojo_rollout_dev fed with the returned U_out gives Z and status bit for bit
  2. the observation is the library's: the contact part of OBS[k] equals dojo_observe_dev's after step k - 1 of a stepwise replay bit for bit; the minimal
                                      part is the joint_max2min source of dojo_maximal_to_minimal_dev in another kernel: bit for bit as well
                                      (measured 0 ulp in both dtypes, where FMA contraction could have differed)
  3. the policy is the formula:       NumPy fp64 on the RECORDED OBS[k]; with `abs` the formula on absolute values,
                                      |U_out - ref| <= 2 (nobs + 4) 2^-53 abs  (+ 2^-23 |ref| for fp32: the one rounding of the result) -- Higham,
                                      Accuracy and Stability of Numerical Algorithms, 3.1: two roundings of the normalisation, an nobs-term dot
                                      product in two summation orders, the bias and feed-forward additions
Shapes: cartpole (Nb 2, nobs 4, the actuated input first), Ant (d.baseline_config(3): nobs 32; act_off 6; contacts observed) at B = 5 (a partly
filled workgroup of four environments) and B = 200 in two groups (spans of 128 and 72), the Ant of the AntARS environment (body contacts too: nobs 37, no
multiple of anything) at B = 5, Atlas at B = 3 (nobs > 64: the strided lanes; the two-wavefront step mapping).  Outputs start as NaN (status: a negative pattern) so that an entry nobody wrote shows; "bit for bit" compares bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import dojo_amd as d
from dojo_amd import api
from gpu_util import dev, same

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -2
H = 4
UNWRITTEN = -123456
# mechanism -> (first driven input, driven inputs (None: all behind act_off), contact forces in the observation)
POLICY = {"cartpole": (0, 1, False), "ant": (6, 8, True), "ant_ars": (6, 8, True), "atlas": (6, None, True)}
K_REFERENCE = np.array([-0.948838, -2.54837, 48.6627, 10.871])      # docs/src/creating_simulation/define_controller.md:23


def _spec(name):
    if name == "ant":
        return d.baseline_config(3)
    if name == "ant_ars":
        return d.get_mechanism("ant")                 # the AntARS environment's: contacts on the bodies as well
    if name == "atlas":
        return d.baseline_config(5)
    if name == "fixed3":
        return d.get_npendulum(num_bodies=3, base_joint_type="Fixed", rest_joint_type="Fixed")
    if name == "sphere_linear":
        return d.get_sphere(contact_type="linear")
    return d.get_mechanism(name)


_handles = {}


def _handle(name, dtype, B):
    key = (name, dtype, B)
    if key not in _handles:
        _handles[key] = api.BatchedMechanism(_spec(name), B, dtype=dtype)
    return _handles[key]


def teardown_module(module):
    for gm in _handles.values():
        gm.close()
    _handles.clear()


def dims(gm, name):
    act_off, na, cf = POLICY[name]
    nu = gm.spec.nu
    na = nu - act_off if na is None else na
    return act_off, na, cf, 2 * nu + (len(gm.spec.contacts) if cf else 0)


_inputs = {}


def inputs(name, dtype, B, steps=H, seed=11):
    """z0 of d.synthetic_inputs; W ~ 0.1 N(0,1) per environment, bias, mean, scale random and nonzero, U_ff = 0.2 N(0,1) on the actuated inputs.  Made once."""
    key = (name, dtype, B, steps, seed)
    if key not in _inputs:
        gm = _handle(name, dtype, B); dt = gm.np_dtype
        act_off, na, cf, nobs = dims(gm, name)
        rng = np.random.default_rng(seed)
        z0 = d.synthetic_inputs(gm.spec, B)[0].astype(dt)
        W = (0.1 * rng.standard_normal((B, na, nobs))).astype(dt)
        bias = (0.1 * rng.standard_normal((B, na))).astype(dt)
        mean = (0.1 * rng.standard_normal(nobs)).astype(dt)
        scale = rng.uniform(0.5, 1.5, nobs).astype(dt)
        U_ff = np.zeros((steps, B, gm.spec.nu), dt)
        U_ff[:, :, act_off:act_off + na] = 0.2 * rng.standard_normal((steps, B, na))
        for a in (z0, W, bias, mean, scale, U_ff):
            a.setflags(write=False)
        _inputs[key] = dict(z0=z0, W=W, bias=bias, mean=mean, scale=scale, U_ff=U_ff)
    return _inputs[key]


def policy_raw(gm, z0, pol, steps, Z, OBS, U, st, handle=True):
    return api.lib().dojo_rollout_policy_dev(gm.h if handle else None, api.addr(z0), None if pol is None else C.byref(pol), int(steps), api.addr(Z), api.addr(OBS), api.addr(U), api.addr(st), api.torch_stream())


def rollout_policy_dev(gm, name, inp, steps=H, want="ZOUS", contact_init=0, per_env=True, act=None):
    """dojo_rollout_policy_dev on NumPy inputs -> dict of NumPy outputs (the ones in `want`; the others are passed as NULL)"""
    B, s = gm.batch, gm.spec
    act_off, na, cf, nobs = dims(gm, name)
    if act is not None:
        act_off, na = act
    tdt = torch.float32 if gm.dtype_code else torch.float64
    keep = {k: dev(inp.get(k)) for k in ("z0", "W", "bias", "mean", "scale", "U_ff")}
    pol = api.DojoPolicy(*[None if keep[k] is None else keep[k].data_ptr() for k in ("W", "bias", "mean", "scale", "U_ff")], int(per_env), act_off, na, int(cf), int(contact_init), 0)
    out = {"Z": torch.full((steps, B, s.nz), float("nan"), dtype=tdt, device="cuda") if "Z" in want else None,
           "O": torch.full((steps + 1, B, nobs), float("nan"), dtype=tdt, device="cuda") if "O" in want else None,
           "U": torch.full((steps, B, s.nu), float("nan"), dtype=tdt, device="cuda") if "U" in want else None,
           "S": torch.full((steps, B), UNWRITTEN, dtype=torch.int32, device="cuda") if "S" in want else None}
    api._chk(policy_raw(gm, keep["z0"], pol, steps, out["Z"], out["O"], out["U"], out["S"]))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def rollout_dev(gm, z0, U):
    """dojo_rollout_dev (open loop) -> Z, status"""
    steps, B = U.shape[:2]
    tdt = torch.float32 if gm.dtype_code else torch.float64
    z0d, Ud = dev(z0), dev(U)
    Z = torch.full((steps, B, gm.spec.nz), float("nan"), dtype=tdt, device="cuda"); st = torch.full((steps, B), UNWRITTEN, dtype=torch.int32, device="cuda")
    api._chk(api.lib().dojo_rollout_dev(gm.h, api.addr(z0d), api.addr(Ud), steps, api.addr(Z), api.addr(st), api.torch_stream()))
    torch.cuda.synchronize()
    return Z.cpu().numpy(), st.cpu().numpy()


def step_observe(gm, z, u, cf, nobs):
    """dojo_step_dev + dojo_observe_dev of the new state -> z_next, obs"""
    tdt = torch.float32 if gm.dtype_code else torch.float64
    zd, ud = dev(z), dev(u)
    zn = torch.empty_like(zd); obs = torch.full((gm.batch, nobs), float("nan"), dtype=tdt, device="cuda")
    api._chk(api.lib().dojo_step_dev(gm.h, api.addr(zd), api.addr(ud), api.addr(zn), None, None, None, None, api.torch_stream()))
    api._chk(api.lib().dojo_observe_dev(gm.h, api.addr(zn), api.addr(obs), int(cf), api.torch_stream()))
    torch.cuda.synchronize()
    return zn.cpu().numpy(), obs.cpu().numpy()


def max2min(gm, z):
    tdt = torch.float32 if gm.dtype_code else torch.float64
    zd = dev(z); x = torch.full((gm.batch, 2 * gm.spec.nu), float("nan"), dtype=tdt, device="cuda")
    api._chk(api.lib().dojo_maximal_to_minimal_dev(gm.h, api.addr(zd), api.addr(x), api.torch_stream()))
    torch.cuda.synchronize()
    return x.cpu().numpy()


_runs = {}


def reference_run(name, dtype, B, groups=None):
    """the closed-loop rollout the three links are checked on: made once per case"""
    key = (name, dtype, B, groups)
    if key not in _runs:
        gm = _handle(name, dtype, B)
        if groups:
            gm.set_groups(groups)
        _runs[key] = rollout_policy_dev(gm, name, inputs(name, dtype, B))
        for a in _runs[key].values():
            a.setflags(write=False)
    return _runs[key]


CASES = [("cartpole", 3, None), ("ant", 5, None), ("ant", 200, 2), ("ant_ars", 5, None), ("atlas", 3, None)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,B,groups", CASES)
def test_every_output_is_written(name, B, groups, dtype):
    r = reference_run(name, dtype, B, groups)
    gm = _handle(name, dtype, B)
    if name == "atlas":
        assert dims(gm, name)[3] > 64                  # the strided lanes of the mat-vec
    if name == "ant_ars":
        assert dims(gm, name)[3] == 37
    assert np.isfinite(r["O"]).all() and np.isfinite(r["U"]).all() and np.isfinite(r["Z"]).all()
    assert (r["S"] != UNWRITTEN).all()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,B,groups", CASES)
def test_steps_consumed_the_recorded_controls(name, B, groups, dtype):
    """link 1"""
    r = reference_run(name, dtype, B, groups)
    gm = _handle(name, dtype, B)
    Z, st = rollout_dev(gm, inputs(name, dtype, B)["z0"], r["U"])
    assert same(Z, r["Z"]) and same(st, r["S"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,B,groups", CASES)
def test_observation_is_the_librarys(name, B, groups, dtype):
    """link 2.  The minimal part was first bounded by 16 ulp of the handle dtype at scale max(1, |ref|) (the same joint_max2min source in two kernels: only
    FMA contraction could differ); measured on MI355X it is 0 ulp in every case and both dtypes, so the assertion is equality."""
    r = reference_run(name, dtype, B, groups)
    gm = _handle(name, dtype, B)
    act_off, na, cf, nobs = dims(gm, name)
    nm = 2 * gm.spec.nu
    z = inputs(name, dtype, B)["z0"]
    eps = float(np.finfo(gm.np_dtype).eps)
    worst, bits = 0.0, True
    for k in range(H + 1):
        ref = max2min(gm, z)
        bits = bits and same(r["O"][k][:, :nm], ref)
        ref = ref.astype(np.float64)
        err = np.abs(r["O"][k][:, :nm].astype(np.float64) - ref) / (eps * np.maximum(1.0, np.abs(ref)))
        worst = max(worst, float(err.max()))
        if k == 0:
            assert same(r["O"][0][:, nm:], np.ones((B, nobs - nm), gm.np_dtype))        # a fresh ContactConstraint
        if k == H:
            break
        zn, obs = step_observe(gm, z, r["U"][k], cf, nobs)
        assert same(zn, r["Z"][k])
        assert same(obs[:, nm:], r["O"][k + 1][:, nm:]), k                               # a clamp of the same impulses
        z = r["Z"][k]
    print("observation vs dojo_maximal_to_minimal_dev, %s %s B=%d: max %.3g ulp" % (name, dtype, B, worst))
    assert bits and worst == 0.0, worst


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_contact_init_takes_the_handles_last_solution(dtype):
    name, B = "ant", 5
    gm = _handle(name, dtype, B)
    act_off, na, cf, nobs = dims(gm, name)
    inp = inputs(name, dtype, B)
    zn, obs = step_observe(gm, inp["z0"], np.zeros((B, gm.spec.nu), gm.np_dtype), cf, nobs)
    r = rollout_policy_dev(gm, name, inp, contact_init=1)
    nm = 2 * gm.spec.nu
    assert same(r["O"][0][:, nm:], obs[:, nm:])
    assert not same(obs[:, nm:], np.ones_like(obs[:, nm:]))
    assert same(r["O"][0][:, :nm], reference_run(name, dtype, B)["O"][0][:, :nm])


def formula(OBS, inp, act_off, na, k, absolute=False):
    f = (lambda a: np.abs(np.asarray(a, np.float64))) if absolute else (lambda a: np.asarray(a, np.float64))
    o, mean = f(OBS[k]), f(inp["mean"])
    oh = ((o + mean) if absolute else (o - mean)) * f(inp["scale"])
    a = f(inp["bias"]) + np.einsum("bij,bj->bi", f(inp["W"]), oh)
    u = f(inp["U_ff"][k]).copy()
    u[:, act_off:act_off + na] += a
    return u


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,B,groups", CASES)
def test_policy_is_the_formula(name, B, groups, dtype):
    """link 3"""
    r = reference_run(name, dtype, B, groups)
    gm = _handle(name, dtype, B)
    act_off, na, cf, nobs = dims(gm, name)
    inp = inputs(name, dtype, B)
    worst = 0.0
    for k in range(H):
        ref, abs_ = formula(r["O"], inp, act_off, na, k), formula(r["O"], inp, act_off, na, k, absolute=True)
        lim = 2.0 * (nobs + 4) * 2.0 ** -53 * abs_ + (2.0 ** -23 * np.abs(ref) if dtype == "f32" else 0.0)
        err = np.abs(r["U"][k].astype(np.float64) - ref)
        worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
        assert (err <= lim).all(), (k, float((err - lim).max()))
        off = np.ones(gm.spec.nu, bool); off[act_off:act_off + na] = False
        assert same(r["U"][k][:, off], inp["U_ff"][k][:, off])
    print("policy vs formula, %s %s B=%d: max error / bound %.3g" % (name, dtype, B, worst))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,B", [("cartpole", 3), ("ant", 5)])
def test_zero_policy_is_the_open_loop(name, B, dtype):
    gm = _handle(name, dtype, B)
    inp = dict(inputs(name, dtype, B))
    inp["W"] = np.zeros_like(inp["W"]); inp["bias"] = np.zeros_like(inp["bias"])
    r = rollout_policy_dev(gm, name, inp)
    assert same(r["U"], inp["U_ff"])
    Z, st = rollout_dev(gm, inp["z0"], inp["U_ff"])
    assert same(r["Z"], Z) and same(r["S"], st)


@pytest.mark.parametrize("per_env", [1, 0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_null_bias_is_the_zero_bias(dtype, per_env):
    """bias = NULL is read as 0.0 in front of the sum: every output is the bits of the run with a bias of zeros"""
    name, B, steps = "cartpole", 3, 3
    gm = _handle(name, dtype, B)
    inp = dict(inputs(name, dtype, B, steps=steps))
    if not per_env:
        inp["W"] = inp["W"][0]
    zeros = dict(inp); zeros["bias"] = np.zeros(inp["W"].shape[:-1], gm.np_dtype)
    null = dict(inp); null["bias"] = None
    a, b = rollout_policy_dev(gm, name, null, steps=steps, per_env=bool(per_env)), rollout_policy_dev(gm, name, zeros, steps=steps, per_env=bool(per_env))
    for k in "ZOUS":
        assert same(a[k], b[k]), k
    assert not same(a["U"], inp["U_ff"])       # (the policy acted)


def test_independence_of_groups_repetition_and_sharing():
    name, dtype, B = "ant", "f32", 200
    gm = _handle(name, dtype, B)
    inp = inputs(name, dtype, B)
    two = reference_run(name, dtype, B, 2)
    gm.set_groups(1)
    one = rollout_policy_dev(gm, name, inp)
    gm.set_groups(2)
    again = rollout_policy_dev(gm, name, inp)
    for k in "ZOUS":
        assert same(one[k], two[k]), k
        assert same(again[k], two[k]), k
    shared = dict(inp); shared["W"] = inp["W"][0]; shared["bias"] = inp["bias"][0]
    tiled = dict(inp); tiled["W"] = np.tile(inp["W"][:1], (B, 1, 1)); tiled["bias"] = np.tile(inp["bias"][:1], (B, 1))
    a, b = rollout_policy_dev(gm, name, shared, per_env=False), rollout_policy_dev(gm, name, tiled, per_env=True)
    for k in "ZOUS":
        assert same(a[k], b[k]), k
    assert not same(a["U"], two["U"])


@pytest.mark.parametrize("name,dtype,B", [("ant", "f32", 5), ("cartpole", "f64", 3)])
def test_null_outputs(name, dtype, B):
    gm = _handle(name, dtype, B)
    inp = inputs(name, dtype, B)
    full = reference_run(name, dtype, B)
    r = rollout_policy_dev(gm, name, inp, want="S")
    assert same(r["S"], full["S"])
    z = np.full((B, gm.spec.nz), np.nan, gm.np_dtype)
    api._chk(api.lib().dojo_get_state(gm.h, api.addr(z)))
    assert same(z, full["Z"][H - 1])
    for leave in "ZOUS":
        r = rollout_policy_dev(gm, name, inp, want="ZOUS".replace(leave, ""))
        assert leave not in r
        for k in r:
            assert same(r[k], full[k]), (leave, k)


@pytest.mark.parametrize("name,dtype,B", [("cartpole", "f64", 3), ("ant", "f32", 5)])
def test_host_variant(name, dtype, B):
    gm = _handle(name, dtype, B)
    inp = inputs(name, dtype, B)
    act_off, na, cf, nobs = dims(gm, name)
    full = reference_run(name, dtype, B)
    Z, OBS, U, st = gm.rollout_policy(inp["z0"], inp["W"], H, bias=inp["bias"], mean=inp["mean"], scale=inp["scale"], U_ff=inp["U_ff"], act_off=act_off, contact_forces=cf)
    assert same(Z, full["Z"]) and same(OBS, full["O"]) and same(U, full["U"]) and same(st, full["S"])


def _refused(gm, rc_want, z0, pol, steps, shapes, handle=True):
    tdt = torch.float32 if gm.dtype_code else torch.float64
    outs = [torch.full(sh, float("nan"), dtype=tdt, device="cuda") for sh in shapes[:3]] + [torch.full(shapes[3], UNWRITTEN, dtype=torch.int32, device="cuda")]
    rc = policy_raw(gm, z0, pol, steps, *outs, handle=handle)
    torch.cuda.synchronize()
    assert rc == rc_want, (rc, rc_want)
    text = gm.last_error() if handle else api.lib().dojo_last_error().decode()
    assert text, "no error text"
    for o in outs[:3]:
        assert bool(torch.isnan(o).all())
    assert bool((outs[3] == UNWRITTEN).all())
    return text


def test_refusals():
    name, dtype, B = "ant", "f64", 5
    gm = api.BatchedMechanism(_spec(name), B, dtype=dtype)        # a fresh handle: no solution yet
    try:
        act_off, na, cf, nobs = dims(gm, name)
        inp = inputs(name, dtype, B)
        nu = gm.spec.nu
        z0, W = dev(inp["z0"]), dev(inp["W"])
        shapes = [(H, B, gm.spec.nz), (H + 1, B, nobs), (H, B, nu), (H, B)]
        pol = lambda **kw: api.DojoPolicy(**{**dict(W=W.data_ptr(), per_env=1, act_off=act_off, na=na, contact_forces=1), **kw})
        _refused(gm, INVALID, z0, pol(), H, shapes, handle=False)
        _refused(gm, INVALID, None, pol(), H, shapes)
        _refused(gm, INVALID, z0, None, H, shapes)
        _refused(gm, INVALID, z0, pol(W=None), H, shapes)
        _refused(gm, INVALID, z0, pol(), 0, shapes)
        _refused(gm, INVALID, z0, pol(na=0), H, shapes)
        _refused(gm, INVALID, z0, pol(act_off=-1), H, shapes)
        _refused(gm, INVALID, z0, pol(act_off=nu - na + 1), H, shapes)
        _refused(gm, INVALID, z0, pol(contact_init=1), H, shapes)
    finally:
        gm.close()
    for mech, code, kw in (("fixed3", INVALID, dict(na=1)), ("fourbar", UNSUPPORTED, dict(na=1)), ("sphere_linear", UNSUPPORTED, dict(na=1, contact_forces=1))):
        gm = api.BatchedMechanism(_spec(mech), 2, dtype="f64")
        try:
            s = gm.spec; nobs = 2 * s.nu + len(s.contacts)
            z0 = torch.zeros((2, s.nz), dtype=torch.float64, device="cuda"); W = torch.zeros((2, 1, max(nobs, 1)), dtype=torch.float64, device="cuda")
            p = api.DojoPolicy(**{**dict(W=W.data_ptr(), per_env=1, act_off=0), **kw})
            _refused(gm, code, z0, p, H, [(H, 2, s.nz), (H + 1, 2, max(nobs, 1)), (H, 2, max(s.nu, 1)), (H, 2)])
        finally:
            gm.close()


def test_cartpole_settles_under_the_reference_gain_in_one_call():
    """the closed loop of docs/src/creating_simulation/define_controller.md:25-52 (u = -K'x on the cart joint, 10 s) as ONE dojo_rollout_policy_dev
    call: thresholds of test_hip_closed_loop_with_the_reference_gain_settles.  The state is carried in maximal coordinates (simulate!), so the oracle is
    driven the same way -- o.step on z directly, o.maximal_to_minimal for the observation (0.0529 at step 1000 for +-pi/4) -- and NOT through
    step_minimal_coordinates!, from which this path differs by up to 1.3e-4 on the oracle itself.  Measured on MI355X: environment 0 agrees
    with that oracle loop to 2.0e-13 over the 1001 observations."""
    from oracle import Oracle
    spec = d.get_cartpole()
    th0 = np.array([np.pi / 4, -np.pi / 4, 0.3, -0.1, 0.6, 0.05, -0.5, 0.0])
    B, steps = len(th0), 1000
    gm = api.BatchedMechanism(spec, B, dtype="f64")
    try:
        X = np.zeros((B, 4)); X[:, 2] = th0
        z0 = gm.minimal_to_maximal(X)
        inp = dict(z0=z0, W=-K_REFERENCE.reshape(1, 4))
        r = rollout_policy_dev(gm, "cartpole", inp, steps=steps, per_env=False)
    finally:
        gm.close()
    OBS = r["O"]
    assert (r["S"] == 0).all()
    assert np.abs(OBS[steps]).max() < 0.1, OBS[steps]
    assert (np.abs(OBS[:, :, 2]).max(axis=0) <= np.abs(th0) + 1e-9).all()
    o = Oracle(spec)
    z = o.minimal_to_maximal(X[0]); worst = 0.0
    for k in range(steps + 1):
        x = o.maximal_to_minimal(z)
        worst = max(worst, float(np.abs(OBS[k][0] - x).max()))
        if k < steps:
            z, info = o.step(z, np.array([-K_REFERENCE @ x, 0.0]))
            assert info["status"] == 0
    print("cartpole closed loop, environment 0 against the oracle driven in maximal coordinates: max |OBS - oracle| = %.3g" % worst)
    assert worst < 1e-6, worst


def test_batched_environment_rollout_policy():
    from dojo_amd.envs import BatchedEnvironment
    B, steps = 4, 3
    env = BatchedEnvironment("ant_ars", B, dtype="f64")
    try:
        na, nobs, nu = env.spec.nu - env.n_unactuated, env.nobs, env.spec.nu
        gen = torch.Generator(device="cuda"); gen.manual_seed(3)
        theta = 0.1 * torch.randn(B, na, nobs, dtype=torch.float64, device="cuda", generator=gen)
        mean = 0.1 * torch.randn(nobs, dtype=torch.float64, device="cuda", generator=gen)
        scale = 0.5 + torch.rand(nobs, dtype=torch.float64, device="cuda", generator=gen)
        env.initialize()
        OBS, U, st = env.rollout_policy(theta, steps, mean=mean, scale=scale)
        torch.cuda.synchronize()
        assert OBS.shape == (steps + 1, B, nobs) and U.shape == (steps, B, nu) and st.shape == (steps, B)
        assert 2 * nu == 28 and nobs > 28 and bool((OBS[0, :, 28:] == 1).all())
        x0 = env.initialize()
        z0 = torch.empty(B, env.spec.nz, dtype=torch.float64, device="cuda")
        api._chk(api.lib().dojo_minimal_to_maximal_dev(env.mechanism.h, api.addr(x0), api.addr(z0), api.torch_stream()))
        O2 = torch.full_like(OBS, float("nan")); U2 = torch.full_like(U, float("nan")); s2 = torch.full_like(st, UNWRITTEN)
        pol = api.DojoPolicy(theta.data_ptr(), None, mean.data_ptr(), scale.data_ptr(), None, 1, env.n_unactuated, na, 1, 0, 0)
        api._chk(policy_raw(env.mechanism, z0, pol, steps, None, O2, U2, s2))
        torch.cuda.synchronize()
        assert same(OBS.cpu().numpy(), O2.cpu().numpy()) and same(U.cpu().numpy(), U2.cpu().numpy()) and same(st.cpu().numpy(), s2.cpu().numpy())
    finally:
        env.close()
