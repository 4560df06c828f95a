#!/usr/bin/env python3
"""Policy optimisation by back-propagation through the closed loop, on the device.

1024 cartpoles near the upright position, one linear state-feedback policy u = W o (o = [y, v_y, theta, omega], the minimal state) shared by all of
them, improved by gradient descent with backtracking on the quadratic cost of the reference's LQR example (Q = I, R = 1,
examples/control/cartpole_lqr.jl)

    cost = mean over the batch of  sum_k |o_k|^2 + u_k^2        over a horizon of H steps

starting from HALF the gain the reference's docs print (docs/src/creating_simulation/define_controller.md: K = [-0.948838, -2.54837, 48.6627,
10.871], u = -K'x).  The gradient w.r.t. the gain comes from ONE reverse sweep through the recorded closed loop
(`dojo_amd.autograd.differentiable_policy_rollout`: dojo_rollout_policy_record_dev forward, dojo_rollout_policy_adjoint_dev backward, the sum over the
batch taken on the device); the reference's learning examples search without gradients (examples/learning/ant_ars.jl).  The cost of every iterate and
its distance to the docs' gain are printed; a finite horizon and a finite set of start states have their own optimum, so the distance shrinks but
need not vanish.  torch owns the tensors, nothing else.

    python examples/cartpole_policy_gradient_device.py [batch] [iterations]          # needs a GPU: libdojo_hip has no CPU fallback
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dojo.jl_amd", "host"))
import dojo_amd as d                                          # noqa: E402
from dojo_amd import api                                      # noqa: E402
from dojo_amd.autograd import differentiable_policy_rollout   # noqa: E402

K_REFERENCE = np.array([-0.948838, -2.54837, 48.6627, 10.871])


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    H = 200                                                                  # 2 s
    torch.cuda.init()                                                        # (torch brings the GPU up first)
    spec = d.get_cartpole()
    gm = api.BatchedMechanism(spec, B, dtype="f64")
    gm.set_gradient_mode(api.GRAD_CONSISTENT)                                # the chain of these Jacobians is the derivative of the rollout
    rng = np.random.default_rng(0)
    X = np.zeros((B, 4)); X[:, 0] = rng.uniform(-0.5, 0.5, B); X[:, 2] = rng.uniform(-0.3, 0.3, B)      # cart offset, pole angle
    z0 = torch.from_numpy(gm.minimal_to_maximal(X)).cuda()
    Kref = torch.from_numpy(K_REFERENCE).cuda()

    def cost(W, grad):
        Wv = W.detach().clone().requires_grad_(grad)
        Z, OBS, U = differentiable_policy_rollout(gm, z0, Wv, steps=H)       # the cart joint is input 0 (act_off = 0, na = 1); the pole joint is passive
        solved = (Z.status == 0).all(dim=0)
        c = ((OBS[:-1] ** 2).sum(dim=(0, 2)) + (U[..., 0] ** 2).sum(dim=0))[solved].mean()
        g = torch.autograd.grad(c, Wv)[0] if grad else None
        return c.item(), g, int(solved.sum())

    W = (-0.5 * Kref).reshape(1, 4).clone()
    step = 1.0
    c, g, ns = cost(W, True)
    for it in range(iters):
        print("iteration %3d   cost %.6f   |K - K_REFERENCE| / |K_REFERENCE| %.4f   K = %s   solved %d / %d"
              % (it, c, ((-W[0] - Kref).norm() / Kref.norm()).item(), np.array2string(-W[0].cpu().numpy(), precision=4), ns, B))
        while True:                                                          # backtracking (Armijo, 1e-4)
            Wn = W - step * g
            cn, _, _ = cost(Wn, False)
            if np.isfinite(cn) and cn <= c - 1e-4 * step * float((g * g).sum()):
                break
            step *= 0.5
            if step < 1e-12:
                print("no descent step left"); gm.close(); return
        W = Wn; step *= 2.0
        c, g, ns = cost(W, True)
    gm.close()


if __name__ == "__main__":
    main()
