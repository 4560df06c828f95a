"""The options of the four reverse sweeps on the GPU -- rollout_adjoint_kernel, rollout_policy_adjoint_kernel, rollout_mlp_adjoint_kernel,
rollout_data_adjoint_kernel and the two reductions -- each against the NumPy recursion and the bound of the module that tests the sweep's main path
(test_rollout_adjoint_gpu, test_policy_adjoint_gpu, test_rollout_mlp_gpu, test_rollout_data_gpu; helpers, cached inputs and handles are theirs):

  a. failed steps at the edges of the horizon: the step that starts the sweep, the step that ends it, two in a row, all, H = 1; any non-zero status;
     fp64 and fp32; per-environment and shared policies; the sums over the batch
  b. state-space cotangents (cot_space = 1) in the closed-loop sweeps, also next to failed steps
  c. the fp32 normalisation q / |q|, on quaternions that are up to 10 % from unit (the un-normalised reference is far outside the bound:
     tests/test_sweep_references.py)
  d. every optional input absent alone; the arrays documented as unread filled with NaN
  e. every subset of the outputs: bit-identical to the run with all outputs, guard elements around every output untouched
  f. data_reduce_kernel with more environments than lanes

The inputs, the failure patterns and the references are tests/sweep_cases.py, checked on their own without a device in tests/test_sweep_references.py."""
import numpy as np
import pytest
import torch

import sweep_cases as S
from gpu_util import dev, guarded, guards_intact, same, tdt_of

pytestmark = pytest.mark.gpu

O, P, N, D = S.O, S.P, S.N, S.D


def teardown_module(module):
    """the handles live in the four modules' caches (whose own teardown may have run already)"""
    for mod in (O, P, N, D):
        for gm in mod._handles.values():
            gm.close()
        mod._handles.clear()


def report(part, what, out, ref, lim):
    print("(%s) %s: largest error / bound = %.3f" % (part, what, S.ratio(out, ref, lim)))


def n_step_of(name, hidden):
    spec = P._spec(name); act_off, na = P.ACT[name]
    return spec.nx + 2 * spec.nu + na + 8 if hidden is None else N.n_step_of(spec, N.widths_of(name, hidden))


def closed_sweep(name, dtype, B, H, inp, hidden, per_env, cot_space=0, outs=None):
    """the affine (hidden None) or the network sweep on the handle of its own module"""
    act_off, na = P.ACT[name]
    if hidden is None:
        return P.sweep(P._handle(name, dtype, B), H, inp, per_env, act_off, na, cot_space, outs=outs)
    return N.mlp_sweep(N._handle(name, dtype, B), H, inp, per_env, act_off, N.widths_of(name, hidden), cot_space, outs=outs)


def closed_check(name, out, ref_inp, hidden, H, f32, per_env, extra=0, abs_G=None):
    spec = P._spec(name); act_off, na = P.ACT[name]
    if hidden is None:
        return P.check_all(spec, out, ref_inp, act_off, na, H, f32, per_env=bool(per_env), extra=extra, abs_G=abs_G)
    return N.check_all(spec, out, ref_inp, act_off, N.widths_of(name, hidden), H, f32, per_env=bool(per_env), extra=extra, abs_G=abs_G)


def closed_report(part, name, out, ref_inp, hidden, H, f32, per_env, extra=0, abs_G=None):
    """the figures behind closed_check (printed, not asserted)"""
    B = np.asarray(ref_inp["G"]).shape[1]
    ref = S.closed_loop_recursion(name, ref_inp, hidden)
    ainp = P.absolute(ref_inp) if abs_G is None else dict(P.absolute(ref_inp), G=abs_G)
    spec = P._spec(name); act_off, na = P.ACT[name]
    abs_ = P.recursion(spec, ainp, act_off, na, absolute=True) if hidden is None else N.recursion(spec, ainp, act_off, N.widths_of(name, hidden), absolute=True)
    for k, v in out.items():
        shared = (not per_env) and k in ("gW", "gbias", "gtheta")
        r, a = (ref[k].sum(0), abs_[k].sum(0)) if shared else (ref[k], abs_[k])
        report(part, "%s %s %s per_env=%d %s" % (name, hidden, "f32" if f32 else "f64", per_env, k), v, r, S.limit(2.0 * (H * (n_step_of(name, hidden) + extra) + (B if shared else 0)), a, r, f32))


CLOSED = [(m, h) for m in S.CLOSED_MECHANISMS for h in (None,) + S.HIDDEN]
closed_ids = lambda v: str(v).replace(" ", "")


# ---------------------------------------------------------------- a. failed steps ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("hb", S.FAILURE_SHAPES)
@pytest.mark.parametrize("name", S.OPEN_MECHANISMS)
def test_failed_steps_open_loop(name, hb, dtype):
    """a. rollout_adjoint_kernel: NaN Jacobians at every failed step; finite, the recursion with the cut, exact zeros where nothing flows (gU at a failed
    step; gz where step 0 failed -- all of environment 4), environment 0 the bits of the call without a status buffer"""
    H, B = hb
    c = S.open_loop_failed(name, dtype, H, B)
    gm = O._handle(name, dtype, B); nx, nu, f32 = gm.spec.nx, gm.spec.nu, dtype == "f32"
    gU, gz = O.adjoint(gm, c["DZ"], c["DU"], c["G"], status=c["status"])
    cU, cz = O.adjoint(gm, *c["clean"])
    (rU, rz), (aU, az) = c["ref"], c["abs"]
    zU, zz = S.open_loop_zero(c["status"])
    report("a", "open-loop %s %s H=%d gz" % (name, dtype, H), gz, rz, S.limit(2.0 * H * (nx + 2), az, rz, f32))
    O.check(gz, rz, az, H, nx, f32, what="gz")
    assert (gz[zz] == 0.0).all() and same(gz[0], cz[0])
    if nu:
        report("a", "open-loop %s %s H=%d gU" % (name, dtype, H), gU, rU, S.limit(2.0 * H * (nx + 2), aU, rU, f32))
        O.check(gU, rU, aU, H, nx, f32, what="gU")
        assert (gU[zU] == 0.0).all() and same(gU[:, 0], cU[:, 0])
    else:
        assert gU is None
    if (H, B) == (4, 6):
        assert (gz[4] == 0.0).all() and (not nu or (gU[:, 4] == 0.0).all())


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("hb", S.FAILURE_SHAPES)
@pytest.mark.parametrize("name,hidden", CLOSED, ids=closed_ids)
def test_failed_steps_closed_loop(name, hidden, hb, dtype):
    """a. rollout_policy_adjoint_kernel (hidden None) and rollout_mlp_adjoint_kernel, one policy per environment and shared (the sums over the batch within the
    bound with n_red = B): finite, the recursion with the cut, gU at a failed step the control cotangent bit for bit, environment 0 the bits of the call
    without a status buffer.  The network sweep's accumulators are first written by step H-1, which has failed in environments 1, 4 and 5."""
    H, B = hb
    f32 = dtype == "f32"
    for per_env in (1, 0):
        clean, bad = S.closed_loop_failed(name, dtype, H, B, hidden, per_env)
        out = closed_sweep(name, dtype, B, H, bad, hidden, per_env)
        ref = closed_sweep(name, dtype, B, H, clean, hidden, per_env)
        closed_report("a", name, out, bad, hidden, H, f32, per_env)
        closed_check(name, out, bad, hidden, H, f32, per_env)
        f = bad["status"] != 0
        assert same(out["gU"][f], np.asarray(bad["G_u"])[f]), per_env
        for k, v in out.items():
            assert np.isfinite(v).all(), (k, per_env)
            if k == "gU":
                assert same(v[:, 0], ref[k][:, 0]), (k, per_env)
            elif per_env or k == "gz":
                assert same(v[0], ref[k][0]), (k, per_env)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("hb", S.FAILURE_SHAPES)
@pytest.mark.parametrize("name", S.DATA_MECHANISMS)
def test_failed_steps_data(name, hb, dtype):
    """a. rollout_data_adjoint_kernel with gtheta_env, gtheta and gz: finite, the recursion with the cut, the shared sum within its bound, exact zeros
    (gz where step 0 failed, gtheta_env where every step failed: environment 4), environment 0 the bits of the call without a status buffer"""
    H, B = hb
    c = S.data_failed(name, dtype, H, B)
    gm = D._handle(name, dtype, B); nx, f32 = gm.spec.nx, dtype == "f32"
    gte, gt, gz = D.data_adjoint(gm, c["DZ"], c["DC"], c["G"], status=c["status"])
    ce, _, cz = D.data_adjoint(gm, *c["clean"])
    (ra, rz), (aa, az) = c["ref"], c["abs"]
    for what, o, r, a in (("gz", gz, rz, az), ("gtheta_env", gte, ra, aa)):
        report("a", "data %s %s H=%d %s" % (name, dtype, H, what), o, r, S.limit(2.0 * H * (nx + 3), a, r, f32))
    D.check(gz, rz, az, H, nx, f32, what="gz"); D.check(gte, ra, aa, H, nx, f32, what="gtheta_env"); D.check_sum(gt, ra, aa, H, nx, f32)
    st = c["status"]
    assert (gz[st[0] != 0] == 0.0).all() and (gte[(st != 0).all(0)] == 0.0).all()
    assert same(gz[0], cz[0]) and same(gte[0], ce[0])
    if (H, B) == (4, 6):
        assert (gz[4] == 0.0).all() and (gte[4] == 0.0).all()


# ---------------------------------------------------------------- b. cot_space = 1 in the closed-loop sweeps ----------------------------------------------------------------
@pytest.mark.parametrize("failed", [False, True], ids=["solved", "failed"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,hidden", CLOSED, ids=closed_ids)
def test_state_space_cotangents_closed_loop(name, hidden, dtype, failed):
    """b. G in state coordinates reaches adjoint::cotangent through the closed-loop kernels' own argument record: Z and G of test_state_space_cotangents, the
    reference through pull_back, ten more operations per step in the bound and pull_back's magnitude sums for |G|; then next to a step that fails at
    k = H-1 (environment 1) and at k = 0 (environment 2) -- the cotangent of a failed step is still fetched"""
    H, B = 3, 5
    f32 = dtype == "f32"
    for per_env in (1, 0):
        dev, ref_inp, Ga = S.closed_loop_state_space(name, dtype, H, B, hidden, per_env, failed=failed)
        out = closed_sweep(name, dtype, B, H, dev, hidden, per_env, cot_space=1)
        closed_report("b", name, out, ref_inp, hidden, H, f32, per_env, extra=10, abs_G=Ga)
        closed_check(name, out, ref_inp, hidden, H, f32, per_env, extra=10, abs_G=Ga)
        if failed:
            f = dev["status"] != 0
            assert same(out["gU"][f], np.asarray(dev["G_u"])[f])


# ---------------------------------------------------------------- c. the fp32 normalisation ----------------------------------------------------------------
C_CASES = [("open", "ant", None), ("data", "ant", None), ("policy", "ant", None), ("mlp", "ant", [17, 5]), ("open", "cartpole", None), ("policy", "cartpole", None)]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,name,hidden", C_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_quaternions_off_the_unit_sphere(kind, name, hidden, dtype):
    """c. cot_space = 1 with every quaternion of Z scaled by a factor from [0.9, 1.1]: an fp32 handle pulls back at q / |q| (the reference normalises; the one
    that does not is at least 100 bounds away), an fp64 handle at q as given (the reference does not normalise; the two references are as far apart)"""
    H, B = 3, 5
    f32 = dtype == "f32"
    assert S.unnormalised_excess(kind, name, H, B, hidden) >= 100.0
    if kind in ("policy", "mlp"):
        dev, ref_inp, Ga = S.closed_loop_state_space(name, dtype, H, B, hidden, scaled=True)
        out = closed_sweep(name, dtype, B, H, dev, hidden, 1, cot_space=1)
        closed_report("c", name, out, ref_inp, hidden, H, f32, 1, extra=10, abs_G=Ga)
        closed_check(name, out, ref_inp, hidden, H, f32, 1, extra=10, abs_G=Ga)
        return
    mod = O if kind == "open" else D
    gm = mod._handle(name, dtype, B); spec = gm.spec; nx = spec.nx
    J0, J1, _ = mod.synthetic(name, dtype, H, B)
    Z, Gs = S.state_cotangents(spec, dtype, H, B, scaled=True)
    Gt, Ga = O.pull_back(Gs, Z, f32)
    ref, abs_ = mod.recursion(J0, J1, Gt), mod.recursion(np.abs(J0), np.abs(J1), Ga)
    if kind == "open":
        out = O.adjoint(gm, J0, J1, Gs, cot_space=1, Z=Z)
        names, extra, check = ("gU", "gz"), 12, O.check
    else:
        gte, gt, gz = D.data_adjoint(gm, J0, J1, Gs, cot_space=1, Z=Z)
        out, names, extra, check = (gte, gz), ("gtheta_env", "gz"), 13, D.check
        D.check_sum(gt, ref[0], abs_[0], H, nx, f32, extra=13)
    for what, o, r, a in zip(names, out, ref, abs_):
        report("c", "%s %s %s %s" % (kind, name, dtype, what), o, r, S.limit(2.0 * H * (nx + extra), a, r, f32))
        check(o, r, a, H, nx, f32, extra=extra, what=what)


# ---------------------------------------------------------------- d. optional inputs, each alone ----------------------------------------------------------------
@pytest.mark.parametrize("absent", ["mean", "scale", "G_u", "G_obs"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,hidden", CLOSED, ids=closed_ids)
def test_optional_inputs_closed_loop(name, hidden, dtype, absent):
    """d. mean, scale, G_u or G_obs NULL, the other three present.  Without G_obs the observation Jacobian of the final state is not read: M[H] is NaN"""
    H, B = 2, 3
    for per_env in (1, 0):
        inp = S.closed_loop_record(name, dtype, H, B, hidden, per_env)
        inp[absent] = None
        if absent == "G_obs":
            inp["M"] = inp["M"].copy(); inp["M"][H] = np.nan
        out = closed_sweep(name, dtype, B, H, inp, hidden, per_env)
        ref_inp = dict(inp, M=np.nan_to_num(inp["M"])) if absent == "G_obs" else inp
        closed_check(name, out, ref_inp, hidden, H, dtype == "f32", per_env)
        assert set(out) == set(P.OUTS if hidden is None else N.OUTS)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["pendulum", "ant"])
def test_optional_buffers_open_loop(name, dtype):
    """d. gz = NULL: step 0 feeds gU alone and DZ[0] is not read (all NaN here); gU = NULL: DU is not read (NULL here)"""
    H, B = 2, 3
    gm = O._handle(name, dtype, B); nx, f32 = gm.spec.nx, dtype == "f32"
    DZ, DU, G = O.synthetic(name, dtype, H, B)
    (rU, rz), (aU, az) = O.recursion(DZ, DU, G), O.recursion(np.abs(DZ), np.abs(DU), np.abs(G))
    DZn = DZ.copy(); DZn[0] = np.nan
    gU, none = O.adjoint(gm, DZn, DU, G, outs={"gU": nan_like(gm, (H, B, gm.spec.nu))})
    assert none is None
    O.check(gU, rU, aU, H, nx, f32, what="gU without gz")
    none, gz = O.adjoint(gm, DZ, None, G, outs={"gz": nan_like(gm, (B, nx))})
    assert none is None
    O.check(gz, rz, az, H, nx, f32, what="gz without gU, DU")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", S.DATA_MECHANISMS)
def test_optional_buffers_data(name, dtype):
    """d. gz alone: DC is not read (all NaN here); gz = NULL: step 0 feeds the accumulators alone and DZ[0] is not read (all NaN here)"""
    H, B = 2, 3
    gm = D._handle(name, dtype, B); nx, f32 = gm.spec.nx, dtype == "f32"
    DZ, DC, G = D.synthetic(name, dtype, H, B)
    (ra, rz), (aa, az) = D.recursion(DZ, DC, G), D.recursion(np.abs(DZ), np.abs(DC), np.abs(G))
    _, _, gz = D.data_adjoint(gm, DZ, np.full_like(DC, np.nan), G, want=("gz",))
    D.check(gz, rz, az, H, nx, f32, what="gz alone")
    DZn = DZ.copy(); DZn[0] = np.nan
    gte, gt, _ = D.data_adjoint(gm, DZn, DC, G, want=("env", "sum"))
    D.check(gte, ra, aa, H, nx, f32, what="gtheta_env without gz"); D.check_sum(gt, ra, aa, H, nx, f32)


def nan_like(gm, shape):
    return torch.full(shape, float("nan"), dtype=torch.float32 if gm.dtype_code else torch.float64, device="cuda")


# ---------------------------------------------------------------- e. output subsets ----------------------------------------------------------------
def subsets(keys, pairs=False):
    import itertools
    return [(k,) for k in keys] + (list(itertools.combinations(keys, 2)) if pairs else [])


def assert_subsets(run, shapes, tdt, pairs=False):
    """run(outs) -> dict of NumPy outputs for the device tensors in outs.  All outputs, then every subset: the same bits, finite, guards untouched"""
    outs = {k: guarded(s, tdt) for k, s in shapes.items()}
    full = run(outs)
    assert set(full) == set(shapes)
    for k, t in outs.items():
        assert guards_intact(t) and np.isfinite(full[k]).all(), k
    for want in subsets(list(shapes), pairs):
        outs = {k: guarded(shapes[k], tdt) for k in want}
        part = run(outs)
        assert set(part) == set(want)
        for k in want:
            assert guards_intact(outs[k]), (want, k)
            assert same(part[k], full[k]), (want, k)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["pendulum", "ant"])
def test_output_subsets_open_loop(name, dtype):
    """e. gU alone (step 0 then starts at column nx: the columns of DU sit on other lanes) and gz alone (DU is not swept) are the bits of the run with both"""
    H, B = 3, 3
    gm = O._handle(name, dtype, B); s = gm.spec
    DZ, DU, G = O.synthetic(name, dtype, H, B)

    def run(outs):
        gU, gz = O.adjoint(gm, DZ, DU, G, outs=outs)
        return {k: v for k, v in (("gU", gU), ("gz", gz)) if v is not None}
    assert_subsets(run, {"gU": (H, B, s.nu), "gz": (B, s.nx)}, tdt_of(gm))


@pytest.mark.parametrize("per_env", [1, 0])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,hidden", CLOSED, ids=closed_ids)
def test_output_subsets_closed_loop(name, hidden, dtype, per_env):
    """e. gW, gbias, gU, gz (affine) and gtheta, gU, gz (network), each alone, one policy per environment and shared"""
    H, B = 3, 3
    inp = S.closed_loop_record(name, dtype, H, B, hidden, per_env)
    act_off, na = P.ACT[name]
    if hidden is None:
        gm = P._handle(name, dtype, B); proto = P.out_tensors(gm, H, per_env, na)
    else:
        gm = N._handle(name, dtype, B); proto = N.mlp_out_tensors(gm, H, per_env, N.widths_of(name, hidden))
    assert_subsets(lambda outs: closed_sweep(name, dtype, B, H, inp, hidden, per_env, outs=outs), {k: tuple(v.shape) for k, v in proto.items()}, tdt_of(gm))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", S.DATA_MECHANISMS)
def test_output_subsets_data(name, dtype):
    """e. gtheta_env, gtheta, gz: each alone and each pair (without gz step 0 starts at column nx; gtheta alone goes through the workspace only)"""
    H, B = 3, 3
    gm = D._handle(name, dtype, B); s = gm.spec
    DZ, DC, G = D.synthetic(name, dtype, H, B)

    def run(outs):
        res = D.data_adjoint(gm, DZ, DC, G, want=tuple(outs), outs=outs)
        return {k: v for k, v in zip(("env", "sum", "gz"), res) if v is not None}
    assert_subsets(run, {"env": (B, D._nth(gm)), "sum": (D._nth(gm),), "gz": (B, s.nx)}, tdt_of(gm), pairs=True)


# ---------------------------------------------------------------- f. data_reduce_kernel beyond one pass ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("B", [257, 600])
def test_data_reduction_over_more_environments_than_lanes(B, dtype):
    """f. sphere, H = 2: lane t of data_reduce_kernel adds the environments t, t + 256, ... -- 257: one lane takes a second, 600: up to three.  gtheta against
    the extended-precision sum of the per-environment reference within check_sum's bound; two runs the same bits; gtheta_env[b] the bits of the
    environment run alone at the lanes' seams"""
    H, name = 2, "sphere"
    gm = D._handle(name, dtype, B); nx, f32 = gm.spec.nx, dtype == "f32"
    DZ, DC, G = D.synthetic(name, dtype, H, B)
    ra, rz = D.recursion(DZ, DC, G)
    aa, az = D.recursion(np.abs(DZ), np.abs(DC), np.abs(G))
    gte, gt, gz = D.data_adjoint(gm, DZ, DC, G)
    gte2, gt2, gz2 = D.data_adjoint(gm, DZ, DC, G)
    assert same(gt, gt2) and same(gte, gte2) and same(gz, gz2)
    ref, asum = D.batch_sum(ra), D.batch_sum(aa)
    import math
    report("f", "sphere %s B=%d gtheta" % (dtype, B), gt, ref, S.limit(2.0 * H * (nx + 3) + math.ceil(math.log2(B)) + 1, asum, ref, f32))
    D.check_sum(gt, ra, aa, H, nx, f32)
    D.check(gte, ra, aa, H, nx, f32, what="gtheta_env"); D.check(gz, rz, az, H, nx, f32, what="gz")
    g1 = D._handle(name, dtype, 1)
    for b in (0, 255, 256, B - 1):
        se, _, sz = D.data_adjoint(g1, DZ[:, b:b + 1], DC[:, b:b + 1], G[:, b:b + 1])
        assert same(se[0], gte[b]) and same(sz[0], gz[b]), b
