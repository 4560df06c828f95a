#!/usr/bin/env python3
"""The line search of an iLQR iteration: T step lengths side by side (include/dojo_hip_linesearch.h) against the loop over them that ilqr._solve drives from the host.

Workload (default): Ant, fp32, H = 20, the controller drives the inputs 6 .. 13 (n = 28, na = 8), P problems from the synthetic start of bench.py with its controls
scaled per step, T = 8 step lengths 1, 1/2, .. (the setup of tools/ilqr_forward_bench.py).  The gains are real ones: one linearization along those controls on a
handle of batch P, the quadratic cost Q = Qf = I, R = I around the start state, and ONE backward pass (dojo_riccati_box_dev, mu = 1, |u| <= 10).
Method: every leg is enqueued on torch's current stream between hipEvents (torch.cuda.Event) after one warm-up of each; `--reps` repetitions, alternating the legs in
one process; the median of each is reported with min .. max.
  (fwd)  ilqr.forward_pass_fused_box            one forward pass on the P-batch handle: the unit
  (fan)  ilqr.rollout_minimal_fan               the T step lengths as one rollout of T P environments on a second handle
  (sel)  ilqr.linesearch_select                 the selection kernel alone: costs, acceptance test, first accepted trial, gather
  (new)  fan + select                           the side-by-side line search
  (a)    T forward_pass_fused_box + torch       all T step lengths one after another with the cost and the torch.where selection of ilqr._solve, no early stop
  (b)    the loop of ilqr._solve                the same with its stop once every problem has accepted (one device-to-host read per trial): the trials a real
                                                iteration from this backward pass takes
Checks: the step length (new) accepts per problem equals (a)'s wherever no trial of the problem lies within 1e-6 max(1, |J|) of its threshold (reported: (a)
evaluates the cost in the handle dtype in torch, (new) in fp64 on the device).  Nothing is gated: the tool reports.  With --out the lines are written to that file
as well.  Needs a GPU: there is no fallback.

    python tools/linesearch_bench.py [--problems 64 256 512] [--trials 8] [--steps 20] [--dtype f32] [--reps 7] [--config 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dojo.jl_amd", "host"))


def measure(a, config, P, T, act_off, na):
    import numpy as np
    import torch
    import dojo_amd as d
    from dojo_amd import api, ilqr

    spec = d.baseline_config(config)
    H, nu = a.steps, spec.nu
    n = 2 * nu
    na = nu - act_off if na is None else na
    gm = api.BatchedMechanism(spec, P, dtype=a.dtype); gmt = api.BatchedMechanism(spec, T * P, dtype=a.dtype)
    tdt = torch.float32 if a.dtype == "f32" else torch.float64
    z0, u = d.synthetic_inputs(spec, P)
    rng = np.random.default_rng(1)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(gm.np_dtype))).cuda()
    x0 = dev(gm.maximal_to_minimal(z0.astype(gm.np_dtype)))
    U = dev(np.stack([u * rng.uniform(0.5, 1.0) for _ in range(H)]))
    eye = lambda k: torch.eye(k, dtype=tdt, device="cuda")
    cost = ilqr.QuadraticCost(Q=eye(n), R=eye(na), Qf=eye(n), x_goal=x0.clone())
    act = slice(act_off, act_off + na)
    c1, alphas = 1e-4, [2.0 ** -t for t in range(T)]
    lo, hi = torch.full((P, na), -10.0, dtype=tdt, device="cuda"), torch.full((P, na), 10.0, dtype=tdt, device="cuda")

    U[:, :, act] = torch.clamp(U[:, :, act], lo, hi)
    X, A, Bm, status = ilqr.linearize_rollout_fused(gm, x0, U)
    mu = torch.ones(P, dtype=tdt, device="cuda")
    K, kff, dV, fail, _, _ = ilqr.riccati_box(gm, A, Bm, *cost.quadratize(X, U[:, :, act])[:4], U, lo, hi, None, mu, status, act_off, na)
    ok = ((status == 0).all(0) & (fail == 0)).to(torch.int32)
    alpha = torch.tensor(alphas, dtype=tdt, device="cuda")[:, None].expand(T, P).contiguous()
    J = cost.value(X, U[:, :, act])
    trials_taken = []

    def host_loop(stop):
        """the line search of ilqr._solve (limits given, no augmented Lagrangian), with or without its early stop"""
        solved = ok != 0
        accepted = torch.zeros(P, dtype=torch.bool, device="cuda"); a_acc = torch.zeros(P, dtype=tdt, device="cuda"); U_new = U.clone()
        count = 0
        for al in alphas:
            Xa, Ua, sa = ilqr.forward_pass_fused_box(gm, X, U, K, kff, float(al), act_off, na, lo, hi)
            Ja = cost.value(Xa, Ua[:, :, act])
            now = ~accepted & solved & (sa == 0).all(0) & (Ja <= J + c1 * (al * dV[:, 0] + al * al * dV[:, 1]))
            U_new = torch.where(now[None, :, None], Ua, U_new); a_acc = torch.where(now, torch.full_like(a_acc, al), a_acc)
            accepted |= now
            count += 1
            if stop and bool((accepted | ~solved).all()):
                break
        if stop:
            trials_taken.append(count)
        return U_new, a_acc

    state = {}

    def fan():
        state["trials"] = ilqr.rollout_minimal_fan(gmt, T, x0, U, X, K, kff, alpha, lo, hi, act_off, na)
        return state["trials"]

    def sel():
        Xt, Ut, st = state["trials"]
        return ilqr.linesearch_select(gmt, T, Xt, Ut, st, alpha, dV, X, U, cost, ok, None, None, c1, act_off, na)

    def new():
        fan()
        return sel()

    legs = [("fwd", lambda: ilqr.forward_pass_fused_box(gm, X, U, K, kff, 0.5, act_off, na, lo, hi)), ("fan", fan), ("sel", sel), ("new", new),
            ("a", lambda: host_loop(False)), ("b", lambda: host_loop(True))]
    out = {}

    def timed(k, f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out[k] = f(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    for k, f in legs:                                                         # one warm-up of each
        out[k] = f()
    torch.cuda.synchronize()
    trials_taken.clear()
    runs = {k: [] for k, _ in legs}
    for _ in range(a.reps):
        for k, f in legs:
            runs[k].append(timed(k, f))
    torch.cuda.synchronize()
    s = out["new"]
    Jc, Jt = s["J_cur"].cpu().numpy(), s["J_trial"].cpu().numpy()
    al = np.array(alphas)[:, None]; dv = dV.double().cpu().numpy()
    thr = Jc[None] + c1 * (al * dv[None, :, 0] + al * al * dv[None, :, 1])
    clear = (np.abs(Jt - thr) >= 1e-6 * np.maximum(1.0, np.abs(Jc))[None]).all(0)
    a_new, a_old = s["alpha"].double().cpu().numpy(), out["a"][1].double().cpu().numpy()
    med = {k: statistics.median(v) for k, v in runs.items()}
    choice = s["choice"].cpu().numpy()
    res = {"tool": "linesearch_bench", "mechanism": spec.name, "dtype": a.dtype, "problems": P, "trials": T, "steps": H, "n": n, "na": na, "act_off": act_off, "reps": a.reps,
           "ms": {k: round(v, 4) for k, v in med.items()}, "ms_runs": {k: [round(t, 4) for t in v] for k, v in runs.items()},
           "trials_of_b": sorted(set(trials_taken)), "accepted_problems": int((choice >= 0).sum()), "choice_histogram": np.bincount(choice + 1, minlength=T + 1).tolist(),
           "riccati_failed": int((fail != 0).sum().item()), "ratio_a_over_new": round(med["a"] / med["new"], 3), "ratio_b_over_new": round(med["b"] / med["new"], 3),
           "ratio_new_over_fwd": round(med["new"] / med["fwd"], 3), "clear_problems": int(clear.sum()), "same_step_length_where_clear": bool((a_new[clear] == a_old[clear]).all())}
    names = {"fwd": "one forward pass (P)    ", "fan": "fan rollout (T P)       ", "sel": "select kernel           ", "new": "fan + select            ",
             "a": "T passes + torch, no stop", "b": "the loop of _solve      "}
    lines = ["%s %s  P = %d  T = %d  H = %d  n = %d  na = %d (inputs %d .. %d)   accepted %d of %d problems, choice histogram (-1, 0, ..) %s; (b) took %s trials; Riccati failures: %d"
             % (spec.name, a.dtype, P, T, H, n, na, act_off, act_off + na - 1, res["accepted_problems"], P, res["choice_histogram"], res["trials_of_b"], res["riccati_failed"])]
    for k, _ in legs:
        lines.append("(%-3s) %s %9.3f ms   (min %.3f .. max %.3f; runs: %s)" % (k, names[k], med[k], min(runs[k]), max(runs[k]), " ".join("%.3f" % t for t in runs[k])))
    lines.append("(new) / (fwd) = %.2f   (a) / (new) = %.2f   (b) / (new) = %.2f   the same step length as (a) on the %d problems with no trial near its threshold: %s"
                 % (res["ratio_new_over_fwd"], res["ratio_a_over_new"], res["ratio_b_over_new"], res["clear_problems"], res["same_step_length_where_clear"]))
    lines.append(json.dumps(res))
    gm.close(); gmt.close()
    del out, state
    torch.cuda.empty_cache()
    return res, lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--problems", type=int, nargs="+", default=[64, 256, 512])
    ap.add_argument("--trials", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--config", type=int, default=3, help="BASELINE.md configuration (3 = Ant, 5 = Atlas)")
    ap.add_argument("--act-off", type=int, default=6)
    ap.add_argument("--na", type=int, default=None, help="driven inputs (default: nu - act_off)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()

    import torch                      # (first: torch brings the GPU up, INTEGRATION.md "Using the library next to PyTorch")
    if not torch.cuda.is_available():
        raise SystemExit("linesearch_bench: no GPU")
    torch.cuda.init()
    lines = []
    for P in a.problems:
        lines += measure(a, a.config, P, a.trials, a.act_off, a.na)[1] + [""]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
