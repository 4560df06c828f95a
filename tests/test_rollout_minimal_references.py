"""The references of the rollout in minimal coordinates, pinned without a device (tests/minimal_cases.py): the NumPy control law the GPU test recomputes U_out with
is the same number in fp64 and in longdouble up to the gate the GPU test applies to the kernel, and the cases' gains do something: on the cartpole, stepped by the
CPU oracle, the closed loop leaves the open loop."""
import numpy as np
import pytest

import minimal_cases as MC
from oracle import Oracle


@pytest.mark.parametrize("shape,H,B", MC.CASES)
def test_law_in_fp64_is_the_longdouble_law_within_the_gate(shape, H, B):
    """X of this check is random of the cases' magnitude (x0 + 0.1 N per step), Xbar = X + 0.05 N: no stepper is needed for the law itself"""
    name, n, nu, act_off, m = MC.SHAPES[shape]
    for f32 in (False, True):
        inp = MC.inputs(shape, H, B, f32)
        rng = np.random.default_rng([7, n, H, B])
        X = inp["x0"][None] + 0.1 * rng.standard_normal((H + 1, B, n)); Xbar = X + 0.05 * rng.standard_normal((H + 1, B, n))
        if f32:
            X, Xbar = (a.astype(np.float32).astype(np.float64) for a in (X, Xbar))
        inp = dict(inp, Xbar=Xbar)
        for k in range(H):
            u64, S = MC.law(inp, k, X[k], act_off, m, np.float64); uld, _ = MC.law(inp, k, X[k], act_off, m, np.longdouble)
            err = np.abs(u64.astype(np.longdouble) - uld).astype(np.float64)
            lim = MC.gate(uld.astype(np.float64), S, n, f32)
            assert (err <= lim).all(), (shape, k, float((err / lim).max()))
            driven = np.zeros(nu, bool); driven[act_off:act_off + m] = True
            assert np.array_equal(u64[:, ~driven], inp["Ubar"][k][:, ~driven])          # the inputs that are not driven are Ubar's, exactly
            assert (np.abs(u64[:, driven] - inp["Ubar"][k][:, driven]) > 0).any()       # ... and the driven ones moved


def test_alpha_is_distinct_per_environment_with_0_and_1():
    a = MC.inputs("ant", 1, 65)["alpha"]
    assert len(set(a.tolist())) == 65 and a[0] == 1.0 and a[1] == 0.0 and ((a >= 0) & (a <= 1)).all()


def test_inputs_of_an_environment_do_not_depend_on_the_batch_or_the_horizon():
    big = MC.inputs("ant", 3, 65)
    for B, H in ((5, 3), (1, 1)):
        small = MC.inputs("ant", H, B)
        for k in ("x0", "xbar0", "alpha"):
            assert np.array_equal(small[k], big[k][:B]), k
        for k in ("Ubar", "K", "kff"):
            assert np.array_equal(small[k], big[k][:H, :B]), k


def _oracle_stepper(spec):
    o = Oracle(spec)

    def step(x, u):
        z, info = o.step(o.minimal_to_maximal(x), u)
        assert info["status"] == 0
        return o.maximal_to_minimal(z)
    return step


def test_cartpole_closed_loop_leaves_the_open_loop():
    """the oracle's step between its coordinate maps, H = 3: with the case's gains the states differ from the open-loop ones by more than 1e-3 -- the feedback term
    of the cases is exercised, not vacuous"""
    shape, H, B = "cartpole1", 3, 5
    name, n, nu, act_off, m = MC.SHAPES[shape]
    step = _oracle_stepper(MC.spec_of(shape))

    def open_loop(x0, U):
        X = [np.asarray(x0)]
        for k in range(U.shape[0]):
            X.append(np.stack([step(X[-1][b], U[k, b]) for b in range(x0.shape[0])]))
        return np.stack(X)

    inp = MC.with_reference(MC.inputs(shape, H, B), open_loop)
    assert np.abs(inp["Xbar"][0] - inp["x0"]).max() > 0
    Xo = open_loop(inp["x0"], inp["Ubar"])
    X = [inp["x0"]]
    for k in range(H):
        u, _ = MC.law(inp, k, X[-1], act_off, m, np.float64)
        X.append(np.stack([step(X[-1][b], u[b]) for b in range(B)]))
    gap = np.abs(np.stack(X) - Xo).max(axis=(0, 2))
    print("cartpole: max |closed - open| per environment", gap)
    assert gap.max() > 1e-3, gap
    assert inp["alpha"][1] == 0.0 and gap[1] > 0          # (environment 1 has no feed-forward step: what moved it is K (x - xbar) alone)
