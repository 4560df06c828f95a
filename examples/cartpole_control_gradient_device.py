#!/usr/bin/env python3
"""Trajectory optimisation by back-propagation through the simulator, on the device.

1024 cartpoles, each with its own target cart position; the force on the cart over a horizon of H steps is improved by gradient descent on

    loss = mean over the batch of  sum_k (y_cart(k) - target)^2 / H  +  (y_cart(H) - target)^2  +  v_cart(H)^2  +  1e-4 sum_k u_k^2

The gradient w.r.t. the whole control sequence comes from ONE reverse sweep over the IFT Jacobians that the rollout recorded
(`dojo_amd.autograd.differentiable_rollout`: dojo_rollout_record_dev forward, dojo_rollout_adjoint_dev backward); the reference's control examples
differentiate a single step (examples/control/cartpole_lqr.jl) or search without gradients.  torch owns the tensors and the optimiser, nothing else.

    python examples/cartpole_control_gradient_device.py [batch] [iterations]          # needs a GPU: libdojo_hip has no CPU fallback
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dojo.jl_amd", "host"))
import dojo_amd as d                                   # noqa: E402
from dojo_amd import api                               # noqa: E402
from dojo_amd.autograd import differentiable_rollout   # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    H = 50                                                                   # 0.5 s
    torch.cuda.init()                                                        # (torch brings the GPU up first)
    spec = d.get_cartpole()
    gm = api.BatchedMechanism(spec, B, dtype="f64")
    gm.set_gradient_mode(api.GRAD_CONSISTENT)                                # the chain of these Jacobians is the derivative of the rollout
    z0 = torch.from_numpy(np.tile(d.initialize(spec), (B, 1))).cuda()        # pole hanging, cart at rest
    target = torch.linspace(-1.0, 1.0, B, dtype=torch.float64, device="cuda")
    force = torch.zeros((H, B), dtype=torch.float64, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([force], lr=0.5)
    for it in range(iters):
        opt.zero_grad()
        U = torch.stack([force, torch.zeros_like(force)], dim=-1)            # [H, B, nu]: the cart's force; the pole joint is passive
        Z = differentiable_rollout(gm, z0, U)                                # [H, B, 26]: cart = Z[..., 0:13], its position along the rail = index 1
        y, vy = Z[..., 1], Z[-1, :, 4]
        solved = (Z.status == 0).all(dim=0)
        per_env = ((y - target) ** 2).mean(dim=0) + (y[-1] - target) ** 2 + vy ** 2 + 1e-4 * (force ** 2).sum(dim=0)
        loss = per_env[solved].mean()
        loss.backward()
        opt.step()
        print("iteration %3d   loss %.6f   worst |y(H) - target| %.4f   solved %d / %d" % (it, loss.item(), (y[-1] - target).abs()[solved].max().item(), int(solved.sum()), B))
    gm.close()


if __name__ == "__main__":
    main()
