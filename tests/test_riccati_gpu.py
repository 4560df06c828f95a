"""The Riccati backward pass on the GPU: dojo_riccati_dev against the recursion it implements (tests/riccati_cases.py, pinned on the CPU by
tests/test_riccati_references.py).  Inputs are synthetic and nothing is stepped: the handles only give the shapes (n = 2 nu).

Gate per output array: |kernel - ref| <= 32 max(e_ref, 2^-52) max|ref| (+ 2^-23 max|ref| for fp32 handles), e_ref = the fp64-against-longdouble distance of the
reference on that case, ref = the longdouble reference.  Measured maxima of |kernel - ref| / (max(e_ref, 2^-52) max|ref|) on MI355X: DESIGN.md section 5h."""
import ctypes as C

import numpy as np
import pytest
import torch

import dojo_amd as d
from dojo_amd import api
from gpu_util import dev, guarded, guards_intact, tdt_of

import riccati_cases as RC

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -2
_handles = {}


def _spec(name):
    if name == "ant":
        return d.baseline_config(3)
    if name == "quadruped":
        return d.baseline_config(4)
    if name == "atlas":
        return d.baseline_config(5)
    return d.get_mechanism(name)


def handle(name, dtype, B):
    """one handle per (mechanism, dtype, batch) for the whole module: the synthetic cases only need its nu"""
    key = (name, dtype, B)
    if key not in _handles:
        _handles[key] = api.BatchedMechanism(_spec(name), B, dtype=dtype)
    return _handles[key]


def teardown_module(module):
    for gm in _handles.values():
        gm.close()
    _handles.clear()


def launch(gm, H, dev_in, outs, act_off, m):
    """dojo_riccati_dev on torch tensors (None = NULL) -> return code"""
    r = api.DojoRiccati(*[api.addr(dev_in.get(k)) for k in ("A", "Bm", "status", "lx", "lu", "lxx", "luu", "lux", "mu")],
                        *[api.addr(outs.get(k)) for k in ("K", "kff", "fail", "dV", "Vx", "Vxx")], int(act_off), int(m))
    return api.lib().dojo_riccati_dev(gm.h, int(H), C.byref(r), api.torch_stream())


def outputs(gm, H, m, omit=()):
    B, n, tdt = gm.batch, 2 * gm.spec.nu, tdt_of(gm)
    shapes = {"K": (H, B, m, n), "kff": (H, B, m), "fail": (B,), "dV": (B, 2), "Vx": (B, n), "Vxx": (B, n, n)}
    return {k: guarded(s, torch.int32 if k == "fail" else tdt) for k, s in shapes.items() if k not in omit}


def run(gm, inp, act_off, m, mu=None, status=None, omit=(), raw=False):
    """NumPy in (inp: the dict of riccati_cases.inputs; lux may be None) -> dict of NumPy outputs (raw: device tensors).  Every output starts as NaN between guard
    elements, which must come back untouched; every element must have been written."""
    H, tdt = inp["A"].shape[0], tdt_of(gm)
    dev_in = {k: dev(v, tdt) for k, v in inp.items()}
    dev_in["mu"] = dev(mu, tdt); dev_in["status"] = dev(status, torch.int32)
    outs = outputs(gm, H, m, omit)
    api._chk(launch(gm, H, dev_in, outs, act_off, m))
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert guards_intact(t), k
    assert not (outs["fail"] == -77).any()
    return outs if raw else {k: t.cpu().numpy().astype(np.float64 if k != "fail" else np.int32) for k, t in outs.items()}


def check(out, ref, e_ref, f32, what):
    """the module's gate on every output array; -> the largest |kernel - ref| / (max(e_ref, 2^-52) max|ref|), which the gate keeps <= 32 (+ the fp32 term)"""
    worst = 0.0
    for k in RC.OUTPUTS:
        if k not in out:
            continue
        err = float(np.abs(out[k] - ref[k]).max()); lim = RC.bound(ref[k], e_ref[k], f32)
        unit = max(e_ref[k], RC.U52) * float(np.abs(ref[k]).max())
        print("%s %s: |kernel - ref| %.3e = %.2f units of max(e_ref, 2^-52) max|ref| (e_ref %.2e), gate %.3e" % (what, k, err, err / unit, e_ref[k], lim))
        assert np.isfinite(out[k]).all(), (what, k)
        assert err <= lim, (what, k, err, lim, e_ref[k])
        worst = max(worst, err / unit)
    return worst


def against_recursion(gm, inp, act_off, m, f32, what, mu=None, status=None):
    """a case outside RC.CASES: both precisions of the reference here"""
    out = run(gm, inp, act_off, m, mu=mu, status=status)
    r64 = RC.recursion(inp, act_off, m, mu=mu, status=status); rld = RC.recursion(inp, act_off, m, mu=mu, status=status, dtype=np.longdouble)
    assert np.array_equal(out["fail"], rld["fail"]) and not rld["fail"].any()
    e = {k: float(np.abs(r64[k] - rld[k]).max() / np.abs(rld[k]).max()) for k in RC.OUTPUTS}
    check(out, {k: rld[k].astype(np.float64) for k in RC.OUTPUTS}, e, f32, what)
    return out


# ---------------------------------------------------------------- 1. kernel = recursion ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape,H,B", RC.CASES)
def test_kernel_matches_the_reference(shape, H, B, dtype):
    """slider (2, 1), cartpole (4, 1) and (4, 2 = nu), ant (28, 8 at offset 6), quadruped (36, 12 at 6), atlas (72, 30 at 6), atlas (72, 5): the 12-accumulator
    build, atlas (72, 36 = nu): the largest plan; H over 1, 3, 20, B over 1, 5, 65.  For fp32 handles the reference sees the inputs rounded to fp32."""
    name, n, nu, act_off, m = RC.SHAPES[shape]
    gm = handle(name, dtype, B)
    assert gm.spec.nu == nu
    inp, ref, e = RC.reference(shape, H, B, dtype == "f32")
    out = run(gm, inp, act_off, m)
    assert not out["fail"].any()
    check(out, ref, e, dtype == "f32", "%s H=%d B=%d %s" % (shape, H, B, dtype))


# ---------------------------------------------------------------- 2. bit identity ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", ["ant", "atlas"])
def test_bit_identical_across_runs_batches_and_places(shape, dtype):
    name, n, nu, act_off, m = RC.SHAPES[shape]
    H, f32 = 3, dtype == "f32"
    big = 65 if shape == "ant" else 5
    full = RC.inputs(shape, H, big, f32)
    a = run(handle(name, dtype, big), full, act_off, m, raw=True)
    b = run(handle(name, dtype, big), full, act_off, m, raw=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # the same environments in another batch, at other places
    for envs in ([big - 1, 0, 3, 1, 2], [big - 1]) if big > 5 else ([4],):
        sub = run(handle(name, dtype, len(envs)), RC.inputs(shape, H, len(envs), f32, envs=envs), act_off, m, raw=True)
        for i, e in enumerate(envs):
            for k in a:
                x, y = (sub[k][:, i], a[k][:, e]) if k in ("K", "kff") else (sub[k][i], a[k][e])
                assert torch.equal(x, y), (k, envs, e)


# ---------------------------------------------------------------- 3. failures ----------------------------------------------------------------
def env_of(out, k, b):
    return out[k][:, b] if k in ("K", "kff") else out[k][b]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_failure_codes_and_zeros(dtype):
    """environment 1 of 3 carries the defect; exact codes, exact zeros, its neighbours bit for bit those of the clean run"""
    name, n, nu, act_off, m = RC.SHAPES["ant"]
    H, B, f32 = 5, 3, dtype == "f32"
    gm = handle(name, dtype, B)
    base = RC.inputs("ant", H, B, f32)
    clean = run(gm, base, act_off, m)
    assert not clean["fail"].any()

    def neighbours_untouched(out):
        for b in (0, 2):
            for k in out:
                assert np.array_equal(env_of(out, k, b), env_of(clean, k, b)), (k, b)

    for kbad in (2, H - 1, 0):           # in the middle, the step that starts the sweep, the step that ends it
        p = {k: v.copy() for k, v in base.items()}; p["luu"][kbad, 1] = -1.0e4 * np.eye(m)
        out = run(gm, p, act_off, m)
        assert out["fail"].tolist() == [0, kbad + 1, 0]
        assert not out["K"][:kbad + 1, 1].any() and not out["kff"][:kbad + 1, 1].any()
        assert np.array_equal(out["K"][kbad + 1:, 1], clean["K"][kbad + 1:, 1]) and np.array_equal(out["kff"][kbad + 1:, 1], clean["kff"][kbad + 1:, 1])
        assert not out["dV"][1].any() and not out["Vx"][1].any() and not out["Vxx"][1].any()
        neighbours_untouched(out)
    # mu cures the indefinite step
    p = {k: v.copy() for k, v in base.items()}; p["luu"][2, 1] = -1.0e4 * np.eye(m)
    against_recursion(gm, p, act_off, m, f32, "cured by mu %s" % dtype, mu=np.array([0.0, 2.0e4, 0.0]))
    # a NaN in A of the solved step 3: Quu of step 3 does not see A_3, its K does; the value function is NaN from there and the pivot of step 2 fails
    p = {k: v.copy() for k, v in base.items()}; p["A"][3, 1, 0, 0] = np.nan
    out = run(gm, p, act_off, m)
    ref = RC.recursion(p, act_off, m)
    assert out["fail"].tolist() == ref["fail"].tolist() == [0, 3, 0]
    assert not out["K"][:3, 1].any() and not out["kff"][:3, 1].any() and np.isnan(out["K"][3, 1]).any()
    assert np.array_equal(out["K"][4, 1], clean["K"][4, 1])
    assert not out["dV"][1].any() and not out["Vx"][1].any() and not out["Vxx"][1].any()
    neighbours_untouched(out)
    # an infinite pivot is a failure too
    p = {k: v.copy() for k, v in base.items()}; p["luu"][1, 1, 0, 0] = np.inf
    assert run(gm, p, act_off, m)["fail"].tolist() == [0, 2, 0]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_failed_steps_are_not_read(dtype):
    """status != 0: the Jacobians of that step are NaN here and count as zero -- the result is the one of zeros there, bit for bit, and the recursion's"""
    name, n, nu, act_off, m = RC.SHAPES["ant"]
    H, B, f32 = 5, 3, dtype == "f32"
    gm = handle(name, dtype, B)
    status = np.zeros((H, B), np.int32); status[4, 0] = 1; status[0, 1] = 2; status[1:3, 2] = -1
    zeros = {k: v.copy() for k, v in RC.inputs("ant", H, B, f32).items()}; nans = {k: v.copy() for k, v in zeros.items()}
    for k in ("A", "Bm"):
        zeros[k][status != 0] = 0.0; nans[k][status != 0] = np.nan
    a = run(gm, zeros, act_off, m)
    b = against_recursion(gm, nans, act_off, m, f32, "failed steps %s" % dtype, status=status)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- 4. optional members ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_optional_member_null_in_turn(dtype):
    name, n, nu, act_off, m = RC.SHAPES["cartpole1"]
    H, B, f32 = 3, 5, dtype == "f32"
    gm = handle(name, dtype, B)
    inp = dict(RC.inputs("cartpole1", H, B, f32))
    mu = np.linspace(0.0, 2.0, B); status = np.zeros((H, B), np.int32); status[1, 2] = 1
    full = run(gm, inp, act_off, m, mu=mu, status=status)
    for omit in ("dV", "Vx", "Vxx"):
        out = run(gm, inp, act_off, m, mu=mu, status=status, omit=(omit,))
        assert set(out) == set(full) - {omit}
        for k in out:
            assert np.array_equal(out[k], full[k]), (omit, k)
    out = run(gm, inp, act_off, m, mu=mu, status=status, omit=("dV", "Vx", "Vxx"))
    assert all(np.array_equal(out[k], full[k]) for k in out)
    # NULL inputs are zeros
    no_lux = dict(inp, lux=None); zero_lux = dict(inp, lux=np.zeros_like(inp["lux"]))
    a, b = run(gm, no_lux, act_off, m, mu=mu, status=status), run(gm, zero_lux, act_off, m, mu=mu, status=status)
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a["K"], full["K"])
    a, b = run(gm, inp, act_off, m, status=status), run(gm, inp, act_off, m, mu=np.zeros(B), status=status)
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a["K"], full["K"])
    a, b = run(gm, inp, act_off, m, mu=mu), run(gm, inp, act_off, m, mu=mu, status=np.zeros((H, B), np.int32))
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a["K"], full["K"])


# ---------------------------------------------------------------- 5. refusals ----------------------------------------------------------------
def refused(gm, H, dev_in, outs, act_off, m, code, text):
    rc = launch(gm, H, dev_in, outs, act_off, m)
    torch.cuda.synchronize()
    assert rc == code, (rc, gm.last_error())
    assert text in gm.last_error(), gm.last_error()
    for k, t in outs.items():
        if t is not None:
            assert guards_intact(t) and bool((t == -77).all() if k == "fail" else torch.isnan(t).all()), k       # nothing was launched


def test_refusals_with_their_text():
    name, n, nu, act_off, m = RC.SHAPES["cartpole1"]
    H, B = 3, 5
    gm = handle(name, "f64", B)
    dev_in = {k: dev(v, torch.float64) for k, v in RC.inputs("cartpole1", H, B).items()}
    outs = outputs(gm, H, m)
    refused(gm, 0, dev_in, outs, act_off, m, INVALID, "dojo_riccati_dev: H must be >= 1")
    for k in ("A", "Bm", "lx", "lu", "lxx", "luu"):
        refused(gm, H, dict(dev_in, **{k: None}), outs, act_off, m, INVALID, "must not be NULL")
    for k in ("K", "kff", "fail"):
        refused(gm, H, dev_in, dict(outs, **{k: None}), act_off, m, INVALID, "must not be NULL")
    for ao, na in ((0, 0), (-1, 1), (1, 2), (2, 1)):
        refused(gm, H, dev_in, outs, ao, na, INVALID, "inside 0 .. nu - 1")
    assert api.lib().dojo_riccati_dev(gm.h, H, None, None) == INVALID
    # the host entry refuses the same way
    r = api.DojoRiccati()
    assert api.lib().dojo_riccati(gm.h, H, C.byref(r)) == INVALID and "dojo_riccati: " in gm.last_error()


def test_refuses_mechanisms_without_inputs_with_loops_and_beyond_the_plan():
    for spec, code, text in ((d.get_npendulum(num_bodies=3, base_joint_type="Fixed", rest_joint_type="Fixed"), INVALID, "no inputs"),
                             (d.get_fourbar(), UNSUPPORTED, "kinematic loop")):
        gm = api.BatchedMechanism(spec, 2, dtype="f64")
        try:
            dummy = torch.zeros(4096, dtype=torch.float64, device="cuda")
            dev_in = {k: dummy for k in ("A", "Bm", "lx", "lu", "lxx", "luu")}
            outs = {k: dummy for k in ("K", "kff")}; outs["fail"] = torch.zeros(2, dtype=torch.int32, device="cuda")
            assert launch(gm, 1, dev_in, outs, 0, 1) == code and text in gm.last_error(), gm.last_error()
            assert not dummy.any()
        finally:
            gm.close()
    # a chain of 40 sliders: n = 80, na = 40 -> n + na = 120 accumulator columns and 80 KB of LDS: refused with the byte count
    spec = d.get_nslider(num_bodies=40)
    gm = api.BatchedMechanism(spec, 1, dtype="f64")
    try:
        n, m = 2 * spec.nu, spec.nu
        assert (n, m) == (80, 40)
        need = 8 * (n * (n + 1) // 2 + max(32 * (n + m), m * n + 2 * m * m) + 2 * n + 4 * m + 8)
        assert need > 65536
        dummy = torch.zeros(80 * 80 * 2, dtype=torch.float64, device="cuda")
        dev_in = {k: dummy for k in ("A", "Bm", "lx", "lu", "lxx", "luu")}
        outs = {k: dummy for k in ("K", "kff")}; outs["fail"] = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert launch(gm, 1, dev_in, outs, 0, m) == UNSUPPORTED
        assert "%d bytes of LDS" % need in gm.last_error(), gm.last_error()
        assert not dummy.any()
    finally:
        gm.close()


# ---------------------------------------------------------------- 6. the host entry ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_host_entry_equals_the_device_entry(dtype):
    name, n, nu, act_off, m = RC.SHAPES["ant"]
    H, B, f32 = 3, 5, dtype == "f32"
    gm = handle(name, dtype, B)
    inp = RC.inputs("ant", H, B, f32)
    mu = np.linspace(0.0, 1.0, B); status = np.zeros((H, B), np.int32); status[1, 3] = 1
    dev = run(gm, inp, act_off, m, mu=mu, status=status)
    K, kff, dV, fail, Vx, Vxx = gm.riccati(inp["A"], inp["Bm"], inp["lx"], inp["lu"], inp["lxx"], inp["luu"], inp["lux"], mu=mu, status=status, act_off=act_off, na=m)
    for k, v in (("K", K), ("kff", kff), ("dV", dV), ("fail", fail), ("Vx", Vx), ("Vxx", Vxx)):
        assert np.array_equal(dev[k], v.astype(dev[k].dtype)), k
    K2, kff2, dV2, fail2 = gm.riccati(inp["A"], inp["Bm"], inp["lx"], inp["lu"], inp["lxx"], inp["luu"], None, act_off=act_off, na=m, value=False)
    assert not fail2.any() and np.isfinite(K2).all()
