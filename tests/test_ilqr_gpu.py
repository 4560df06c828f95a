"""Batched iLQR on the GPU (dojo_amd/ilqr.py: linearize_rollout, riccati, the closed-loop forward pass, the per-environment line search and regularisation).

Slider: one step is affine in the minimal coordinates, so the problem is linear-quadratic and ONE iteration with step length 1 is the optimum: the second
backward pass predicts no further change.  Measured ratio |dV[0] + dV[1]| second / first: DESIGN.md section 5h.
Cartpole: the cost of every environment never rises and ends below the start."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import dojo_amd as d
from dojo_amd import api, ilqr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV, DT = "cuda", torch.float64


def t(a):
    return torch.tensor(a, dtype=DT, device=DEV)


def test_slider_is_solved_by_one_iteration():
    B, H = 3, 10
    spec = d.get_mechanism("slider")
    gm = api.BatchedMechanism(spec, B, dtype="f64", opts=d.SolverOptions(rtol=1e-10, btol=1e-10))
    try:
        x0 = t([[0.0, 0.0], [0.3, -0.5], [-0.2, 1.0]])
        U0 = torch.zeros((H, B, 1), dtype=DT, device=DEV)
        cost = ilqr.QuadraticCost(Q=torch.eye(2, dtype=DT, device=DEV), R=0.1 * torch.eye(1, dtype=DT, device=DEV), Qf=10.0 * torch.eye(2, dtype=DT, device=DEV),
                                  x_goal=t([0.5, 0.0]))
        res = ilqr.solve(gm, x0, U0, cost, 2)
        torch.cuda.synchronize()
        assert not res["fail"].any()
        assert (res["a"][0] == 1.0).all(), res["a"]
        dV = res["dV"].cpu().numpy()
        first, second = np.abs(dV[0].sum(-1)), np.abs(dV[1].sum(-1))
        print("slider: |dV[0] + dV[1]| first %s, second %s, ratio %s" % (first, second, second / first))
        assert (first > 0).all() and (second <= 1e-6 * first).all(), (first, second)
        J = res["J"].cpu().numpy()
        assert (J[1] < J[0]).all() and (np.abs(J[2] - J[1]) <= 1e-6 * np.abs(J[0] - J[1])).all()
        # the model was exact: the actual change of the first iteration is the predicted one
        assert np.allclose(J[1] - J[0], dV[0].sum(-1), rtol=1e-6)
    finally:
        gm.close()


def test_cartpole_costs_fall_per_environment():
    B, H, iters = 4, 30, 6
    spec = d.get_cartpole()
    gm = api.BatchedMechanism(spec, B, dtype="f64", opts=d.SolverOptions(rtol=1e-8, btol=1e-8))
    try:
        x0 = torch.zeros((B, 4), dtype=DT, device=DEV); x0[:, 2] = t([0.2, 0.6, 1.5, np.pi])
        U0 = torch.zeros((H, B, 2), dtype=DT, device=DEV)
        cost = ilqr.QuadraticCost(Q=0.01 * torch.eye(4, dtype=DT, device=DEV), R=1e-4 * torch.eye(1, dtype=DT, device=DEV), Qf=10.0 * torch.eye(4, dtype=DT, device=DEV),
                                  x_goal=torch.zeros(4, dtype=DT, device=DEV))
        res = ilqr.solve(gm, x0, U0, cost, iters, act_off=0, na=1)
        torch.cuda.synchronize()
        J = res["J"].cpu().numpy()
        print("cartpole J per iteration:\n%s\naccepted a:\n%s" % (J, res["a"].cpu().numpy()))
        assert J.shape == (iters + 1, B) and np.isfinite(J).all()
        assert (np.diff(J, axis=0) <= 0).all(), J
        assert (J[-1] < J[0]).all(), J
        assert not res["fail"][-1].any()
        assert not res["U"][:, :, 1].any()                 # the pole's input is not driven
    finally:
        gm.close()


def test_example_runs_at_a_small_batch():
    spec = importlib.util.spec_from_file_location("cartpole_ilqr_device", os.path.join(ROOT, "examples", "cartpole_ilqr_device.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    res = mod.main(["3", "20", "3"])
    J = res["J"].cpu().numpy()
    assert J.shape == (4, 3) and (J[-1] < J[0]).all()
