#!/usr/bin/env python3
"""Optimisation of a neural controller by back-propagation through the closed loop, on the device.

1024 cartpoles near the upright position, one small tanh network u = b_2 + W_2 tanh(b_1 + W_1 o) (o = [y, v_y, theta, omega], the minimal state;
a torch.nn.Sequential of two Linear layers) shared by all of them, improved by gradient descent with backtracking on the quadratic cost of the
reference's LQR example (Q = I, R = 1, examples/control/cartpole_lqr.jl)

    cost = mean over the batch of  sum_k |o_k|^2 + u_k^2        over a horizon of H steps.

The network starts as a stabilising but poor controller: its first layer reads HALF the gain the reference's docs print
(docs/src/creating_simulation/define_controller.md) into one hidden unit scaled to tanh's linear range, the other units start small and random.  The
gradient w.r.t. every parameter comes from ONE reverse sweep through the recorded closed loop (`dojo_amd.autograd.differentiable_mlp_rollout`:
dojo_rollout_mlp_record_dev forward, dojo_rollout_mlp_adjoint_dev backward, the sum over the batch taken on the device) and reaches the modules'
parameters through the torch.cat that lays them out as the ABI's theta.  The loss before and after is printed.  torch owns the tensors and the
optimisation loop, nothing else.

    python examples/cartpole_mlp_policy_gradient_device.py [batch] [iterations] [hidden]          # needs a GPU: libdojo_hip has no CPU fallback
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dojo.jl_amd", "host"))
import dojo_amd as d                                          # noqa: E402
from dojo_amd import api                                      # noqa: E402
from dojo_amd.autograd import differentiable_mlp_rollout      # noqa: E402

K_REFERENCE = np.array([-0.948838, -2.54837, 48.6627, 10.871])


def flat(net):
    """the parameters of a Sequential of Linear layers (with Tanh between them) in the layout of api.pack_mlp: per layer the row-major weight, then the bias"""
    return torch.cat([t.reshape(-1) for m in net if isinstance(m, torch.nn.Linear) for t in (m.weight, m.bias)])


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    nhid = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    H = 200                                                                  # 2 s
    torch.cuda.init()                                                        # (torch brings the GPU up first)
    spec = d.get_cartpole()
    gm = api.BatchedMechanism(spec, B, dtype="f64")
    gm.set_gradient_mode(api.GRAD_CONSISTENT)                                # the chain of these Jacobians is the derivative of the rollout
    rng = np.random.default_rng(0)
    X = np.zeros((B, 4)); X[:, 0] = rng.uniform(-0.5, 0.5, B); X[:, 2] = rng.uniform(-0.3, 0.3, B)      # cart offset, pole angle
    z0 = torch.from_numpy(gm.minimal_to_maximal(X)).cuda()
    widths = [4, nhid, 1]
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(4, nhid), torch.nn.Tanh(), torch.nn.Linear(nhid, 1)).double().cuda()
    with torch.no_grad():
        s = 0.02                                                             # unit 0: tanh(s K'o / 2) / s ~ K'o / 2 while |s K'o| << 1
        for p in net.parameters():
            p.mul_(0.01)
        net[0].weight[0] = torch.from_numpy(-0.5 * s * K_REFERENCE).cuda(); net[0].bias[0] = 0.0
        net[2].weight[0, 0] = 1.0 / s
    params = list(net.parameters())

    def cost(grad):
        Z, OBS, U = differentiable_mlp_rollout(gm, z0, flat(net), widths, steps=H)       # the cart joint is input 0 (act_off = 0, na = 1); the pole joint is passive
        solved = (Z.status == 0).all(dim=0)
        c = ((OBS[:-1] ** 2).sum(dim=(0, 2)) + (U[..., 0] ** 2).sum(dim=0))[solved].mean()
        g = torch.autograd.grad(c, params) if grad else None
        return c.item(), g, int(solved.sum())

    step = 1e-3
    c, g, ns = cost(True)
    first = c
    for it in range(iters):
        print("iteration %3d   cost %.6f   |grad| %.3e   solved %d / %d" % (it, c, float(sum((x * x).sum() for x in g)) ** 0.5, ns, B))
        old = [p.detach().clone() for p in params]
        gg = float(sum((x * x).sum() for x in g))
        while True:                                                          # backtracking (Armijo, 1e-4)
            with torch.no_grad():
                for p, o, x in zip(params, old, g):
                    p.copy_(o - step * x)
                cn, _, _ = cost(False)
            if np.isfinite(cn) and cn <= c - 1e-4 * step * gg:
                break
            step *= 0.5
            if step < 1e-14:
                with torch.no_grad():
                    for p, o in zip(params, old):
                        p.copy_(o)
                print("no descent step left")
                print("loss before %.6f   after %.6f" % (first, c)); gm.close(); return
        step *= 2.0
        c, g, ns = cost(True)
    print("loss before %.6f   after %.6f   (%d gradient steps, %d parameters)" % (first, c, iters, sum(p.numel() for p in params)))
    gm.close()


if __name__ == "__main__":
    main()
