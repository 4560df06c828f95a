#!/usr/bin/env python3
"""Trajectory optimisation with iLQR on the device: swing-up of B cartpoles from different start angles in ONE batch.

The reference's examples/trajectory_optimization run IterativeLQR over get_minimal_gradients! for one mechanism.  Here every environment has its own
trajectory, its own regularisation and its own line search, and every stage is one call for the whole batch:

    linearize_rollout   H calls of dojo_minimal_gradients_dev (the step and its Jacobians in minimal coordinates, on the GPU)
    riccati             ONE launch of dojo_riccati_dev: the backward pass of all H steps of all environments (csrc/dojo_riccati.hpp)
    forward_pass        H calls of dojo_step_minimal_dev per trial step length, the feedback law evaluated in torch between them

The cart's input is the only driven one (act_off = 0, na = 1); the minimal state is [cart position, cart velocity, pole angle, pole angular velocity], the pole is
upright at angle 0 and hangs at pi.

With --fused the first and the last stage are ONE call of dojo_rollout_minimal_dev each (ilqr.linearize_rollout_fused, ilqr.forward_pass_fused): the steps, the
feedback law and the Jacobians of the whole horizon on the device, every environment group at its own pace.

With --limit F the swing-up runs under |u| <= F (ilqr.solve_limited, control-limited DDP: include/dojo_hip_limits.h): the backward pass is ONE launch of
dojo_riccati_box_dev (a box QP per step, the gain rows of clamped inputs zero), the forward pass clamps; the largest |u| and the share of steps at the bound are
printed.

With --goal the swing-up ends AT the upright state instead of near it (ilqr.solve_constrained, IterativeLQR's augmented-Lagrangian loop:
include/dojo_hip_constraints.h): a terminal goal constraint x_H = 0 with a modest terminal cost (Qf = Q) in place of the large one, 4 outer iterations of
[iterations] / 4 inner ones each; the backward pass is ONE launch of dojo_riccati_al_dev, which adds the constraint's terms to the step's model inside the kernel.
The terminal violation max |x_H| is printed per outer iteration next to that of `solve` under the same cost and as many iterations.  --limit F combines with it.

With --side-by-side the line search runs side by side (ilqr.solve_side_by_side, include/dojo_hip_linesearch.h): a second handle of 8 x batch environments rolls
out all eight step lengths of every cartpole in ONE call of dojo_rollout_minimal_fan_dev, and ONE launch of dojo_linesearch_select_dev evaluates the costs, applies
the acceptance test and gathers the first accepted trial; the host reads nothing back during the iterations.  It pays when an iteration needs two or more step lengths; where every cartpole accepts the full step it costs more than the loop it replaces (DESIGN.md 5l has the measurements).
--limit F combines with it; --goal does not.

    python examples/cartpole_ilqr_device.py [batch] [horizon] [iterations] [--fused] [--limit F] [--goal] [--side-by-side]     # needs a GPU: libdojo_hip has no CPU fallback
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dojo.jl_amd", "host"))
import dojo_amd as d                                   # noqa: E402
from dojo_amd import api, ilqr                         # noqa: E402


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    fused = "--fused" in argv; argv = [a for a in argv if a != "--fused"]
    goal = "--goal" in argv; argv = [a for a in argv if a != "--goal"]
    side = "--side-by-side" in argv; argv = [a for a in argv if a != "--side-by-side"]
    if side and goal:
        raise SystemExit("--side-by-side does not combine with --goal (constraints in the side-by-side driver are not built)")
    limit = None
    if "--limit" in argv:
        i = argv.index("--limit"); limit = float(argv[i + 1]); del argv[i:i + 2]
    B = int(argv[0]) if len(argv) > 0 else 64
    H = int(argv[1]) if len(argv) > 1 else 60
    iters = int(argv[2]) if len(argv) > 2 else 40
    torch.cuda.init()                                  # (torch brings the GPU up first: INTEGRATION.md "Using the library next to PyTorch")
    spec = d.get_cartpole(timestep=0.05)
    gm = api.BatchedMechanism(spec, B, dtype="f64", opts=d.SolverOptions(rtol=1e-8, btol=1e-8))
    dev, dt = torch.device("cuda"), torch.float64
    # the starts: hanging, and a spread of angles around it
    x0 = torch.zeros((B, 4), dtype=dt, device=dev)
    x0[:, 2] = torch.linspace(np.pi, 0.5 * np.pi, B, dtype=dt, device=dev)
    U0 = torch.zeros((H, B, spec.nu), dtype=dt, device=dev)
    cost = ilqr.QuadraticCost(Q=torch.diag(torch.tensor([1.0, 0.1, 1.0, 0.1], dtype=dt, device=dev)) * spec.timestep,
                              R=torch.eye(1, dtype=dt, device=dev) * 0.01 * spec.timestep,
                              Qf=torch.diag(torch.tensor([1.0, 0.1, 1.0, 0.1] if goal else [100.0, 10.0, 100.0, 10.0], dtype=dt, device=dev)),
                              x_goal=torch.zeros(4, dtype=dt, device=dev))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if side:
        trials = 8                                     # the step lengths 1, 1/2, .. 1/128 of ilqr.solve
        gmt = api.BatchedMechanism(spec, trials * B, dtype="f64", opts=d.SolverOptions(rtol=1e-8, btol=1e-8))
        lim = (None, None) if limit is None else (-limit, limit)
        res = ilqr.solve_side_by_side(gm, gmt, x0, U0, cost, iters, lim[0], lim[1], act_off=0, na=1)
        gmt.close()
    elif goal:
        outer = 4; inner = max(1, iters // outer)
        lim = {} if limit is None else {"lo": -limit, "hi": limit}
        res = ilqr.solve_constrained(gm, x0, U0, cost, ilqr.GoalConstraint(torch.zeros(4, dtype=dt, device=dev)), inner, outer, act_off=0, na=1, fused=fused, **lim)
    elif limit is None:
        res = ilqr.solve(gm, x0, U0, cost, iters, act_off=0, na=1, fused=fused)
    else:
        res = ilqr.solve_limited(gm, x0, U0, cost, iters, -limit, limit, act_off=0, na=1, fused=fused)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    J = res["J"].cpu().numpy()
    for i in range(J.shape[0]):
        print("iteration %2d: cost min %.4e  median %.4e  max %.4e" % (i, J[i].min(), np.median(J[i]), J[i].max()) +
              ("" if i == J.shape[0] - 1 else "   accepted %d / %d, mu max %.1e" % (int((res["a"][i] > 0).sum()), B, float(res["mu"][i].max()))))
    xH = res["X"][-1].cpu().numpy()
    print("final |pole angle|: min %.3f  median %.3f  max %.3f rad (start: %.3f .. %.3f)" % (np.abs(xH[:, 2]).min(), np.median(np.abs(xH[:, 2])), np.abs(xH[:, 2]).max(), 0.5 * np.pi, np.pi))
    if limit is not None:
        u = res["U"][:, :, 0].abs()
        print("|u| <= %g: largest |u| %.6g, %.1f %% of the %d environment-steps at the bound" % (limit, float(u.max()), 100.0 * float((u == limit).double().mean()), u.numel()))
        assert float(u.max()) <= limit
    if goal:
        free = (ilqr.solve(gm, x0, U0, cost, inner * outer, act_off=0, na=1, fused=fused) if limit is None else
                ilqr.solve_limited(gm, x0, U0, cost, inner * outer, -limit, limit, act_off=0, na=1, fused=fused))
        dist = free["X"][-1].abs().amax(1).cpu().numpy()
        viol = res["viol"].cpu().numpy()
        for o in range(viol.shape[0]):
            print("outer %d: terminal violation max |x_H - goal|  min %.3e  median %.3e  max %.3e%s" % (o, viol[o].min(), np.median(viol[o]), viol[o].max(), "   (the start)" if o == 0 else ""))
        print("without the constraint, same cost, %d iterations:    min %.3e  median %.3e  max %.3e" % (inner * outer, dist.min(), np.median(dist), dist.max()))
        print("rho %.1e, largest |lambda| %.3e" % (float(res["rho"].max()), float(res["lam"].abs().max())))
    if side:
        ch = res["choice"].cpu().numpy()
        print("line search side by side: accepted trial per iteration, mean %.2f, largest %d, none %d of %d" % (ch[ch >= 0].mean() if (ch >= 0).any() else -1, ch.max(), int((ch < 0).sum()), ch.size))
    print("%d environments x %d steps x %d iterations in %.2f s%s" % (B, H, iters, el, " (line search side by side)" if side else " (fused rollouts)" if fused else ""))
    assert goal or (J[-1] <= J[0]).all()                # (under a goal constraint the cost alone may rise: the merit is what falls)
    gm.close()
    return res


if __name__ == "__main__":
    main()
