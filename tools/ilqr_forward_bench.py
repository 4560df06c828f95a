#!/usr/bin/env python3
"""The two rollouts of an iLQR iteration, stepwise from Python against one call of dojo_rollout_minimal_dev (include/dojo_hip_trajopt.h).

Workload (default): Ant, fp32, B = 4096, H = 20, the controller drives the inputs 6 .. 13 (n = 28, na = 8), from the synthetic start of bench.py with its controls
scaled per step.  The gains are real ones: one linearization along those controls, the quadratic cost Q = Qf = I, R = I around the start state, and ONE backward pass
(dojo_riccati_dev, mu = 1); the forward passes run with the step length 0.5.
Method: every leg is enqueued on torch's current stream between hipEvents (torch.cuda.Event) after one warm-up of each; `--reps` repetitions, alternating the four
legs in one process; the median of each is reported with min .. max.
  (a)  ilqr.linearize_rollout        H calls of dojo_minimal_gradients_dev
  (a') ilqr.linearize_rollout_fused  one call, Jacobians recorded
  (b)  ilqr.forward_pass             H rounds of torch einsum + dojo_step_minimal_dev
  (b') ilqr.forward_pass_fused       one call
The stepwise legs are the reference.  Checks: (a') returns the bits of (a); X of (b') is compared with X of (b) (reported: (b) evaluates the feedback law in the
handle dtype in torch, (b') in fp64 on the device).
Condition (the tool exits with status 1 when it is missed): (a') <= (a) and (b') <= (b), each with the spread (max - min) of the stepwise leg in this run as margin.
A second workload (default: Atlas, B = 2048) is reported only.  With --out the lines are written to that file as well.  Needs a GPU: there is no fallback.

    python tools/ilqr_forward_bench.py [--batch 4096] [--steps 20] [--dtype f32] [--reps 7] [--config 3] [--second-config 5 --second-batch 2048] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dojo.jl_amd", "host"))


def measure(a, config, B, act_off, na, gated):
    import numpy as np
    import torch
    import dojo_amd as d
    from dojo_amd import api, ilqr

    spec = d.baseline_config(config)
    H, nu = a.steps, spec.nu
    n = 2 * nu
    na = nu - act_off if na is None else na
    gm = api.BatchedMechanism(spec, B, dtype=a.dtype)
    tdt = torch.float32 if a.dtype == "f32" else torch.float64
    z0, u = d.synthetic_inputs(spec, B)
    rng = np.random.default_rng(1)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(gm.np_dtype))).cuda()
    x0 = dev(gm.maximal_to_minimal(z0.astype(gm.np_dtype)))
    U = dev(np.stack([u * rng.uniform(0.5, 1.0) for _ in range(H)]))
    eye = lambda k: torch.eye(k, dtype=tdt, device="cuda")
    cost = ilqr.QuadraticCost(Q=eye(n), R=eye(na), Qf=eye(n), x_goal=x0.clone())
    act = slice(act_off, act_off + na)

    out = {}
    X, A, Bm, status = ilqr.linearize_rollout(gm, x0, U)                      # (warm-up of (a), and the record the gains come from)
    mu = torch.ones(B, dtype=tdt, device="cuda")
    K, kff, dV, fail = ilqr.riccati(gm, A, Bm, *cost.quadratize(X, U[:, :, act]), mu, status, act_off, na)
    alpha = torch.full((B,), 0.5, dtype=tdt, device="cuda")
    legs = [("a", lambda: ilqr.linearize_rollout(gm, x0, U)), ("a'", lambda: ilqr.linearize_rollout_fused(gm, x0, U)),
            ("b", lambda: ilqr.forward_pass(gm, X, U, K, kff, 0.5, act_off, na)), ("b'", lambda: ilqr.forward_pass_fused(gm, X, U, K, kff, alpha, act_off, na))]

    def timed(k, f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out[k] = f(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    for k, f in legs:                                                         # one warm-up of each
        out[k] = f()
    torch.cuda.synchronize()
    runs = {k: [] for k, _ in legs}
    for _ in range(a.reps):
        for k, f in legs:
            runs[k].append(timed(k, f))
    torch.cuda.synchronize()
    same_a = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(out["a"], out["a'"]))
    both = (out["b"][2] == 0).all(0) & (out["b'"][2] == 0).all(0)
    diff_b = float((out["b"][0].double() - out["b'"][0].double())[:, both].abs().max().item()) if bool(both.any()) else float("nan")
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = {k: max(v) - min(v) for k, v in runs.items()}
    res = {"tool": "ilqr_forward_bench", "mechanism": spec.name, "dtype": a.dtype, "batch": B, "steps": H, "n": n, "na": na, "act_off": act_off, "reps": a.reps,
           "env_steps": H * B, "solved_env_steps": {k: int((out[k][3 if k.startswith("a") else 2] == 0).sum().item()) for k, _ in legs},
           "riccati_failed_envs": int((fail != 0).sum().item()),
           "ms": {k: round(v, 4) for k, v in med.items()}, "ms_runs": {k: [round(t, 4) for t in v] for k, v in runs.items()},
           "spread_ms": {k: round(v, 4) for k, v in spread.items()}, "ratio_a_over_a_fused": round(med["a"] / med["a'"], 3), "ratio_b_over_b_fused": round(med["b"] / med["b'"], 3),
           "menv_steps_per_s": {k: round(H * B / med[k] / 1e3, 4) for k, _ in legs},
           "linearize_fused_bit_identical": bool(same_a), "forward_fused_vs_stepwise_max_abs_dX": diff_b, "gated": gated}
    res["condition_a"] = bool(med["a'"] <= med["a"] + spread["a"]); res["condition_b"] = bool(med["b'"] <= med["b"] + spread["b"])
    names = {"a": "linearize_rollout       ", "a'": "linearize_rollout_fused ", "b": "forward_pass            ", "b'": "forward_pass_fused      "}
    lines = ["%s %s  B = %d  H = %d  n = %d  na = %d (inputs %d .. %d)   solved environment-steps of %d: %s; Riccati failures: %d environments"
             % (spec.name, a.dtype, B, H, n, na, act_off, act_off + na - 1, H * B, " ".join("(%s) %d" % kv for kv in res["solved_env_steps"].items()), res["riccati_failed_envs"])]
    for k, _ in legs:
        lines.append("(%-2s) %s %9.3f ms  %6.3f M env-steps/s   (min %.3f .. max %.3f; runs: %s)"
                     % (k, names[k], med[k], res["menv_steps_per_s"][k], min(runs[k]), max(runs[k]), " ".join("%.3f" % t for t in runs[k])))
    tail = "" if gated else "   (reported only)"
    lines.append("(a) / (a') = %.2f   (a') <= (a) within the spread of (a) (%.3f ms): %s%s" % (res["ratio_a_over_a_fused"], spread["a"], "met" if res["condition_a"] else "MISSED", tail))
    lines.append("(b) / (b') = %.2f   (b') <= (b) within the spread of (b) (%.3f ms): %s%s" % (res["ratio_b_over_b_fused"], spread["b"], "met" if res["condition_b"] else "MISSED", tail))
    lines.append("(a') returns the bits of (a): %s;  max |X(b') - X(b)| over the environments both solved: %.2e   (reported: the law is fp64 on the device in (b'))" % (same_a, diff_b))
    lines.append(json.dumps(res))
    gm.close()
    del out
    torch.cuda.empty_cache()
    return res, lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--config", type=int, default=3, help="BASELINE.md configuration (3 = Ant)")
    ap.add_argument("--act-off", type=int, default=6)
    ap.add_argument("--na", type=int, default=None, help="driven inputs (default: nu - act_off)")
    ap.add_argument("--second-config", type=int, default=5, help="reported only (5 = Atlas; 0 = none)")
    ap.add_argument("--second-batch", type=int, default=2048)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()

    import torch                      # (first: torch brings the GPU up, INTEGRATION.md "Using the library next to PyTorch")
    if not torch.cuda.is_available():
        raise SystemExit("ilqr_forward_bench: no GPU")
    torch.cuda.init()
    res, lines = measure(a, a.config, a.batch, a.act_off, a.na, True)
    if a.second_config:
        _, more = measure(a, a.second_config, a.second_batch, 6, None, False)
        lines += [""] + more
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if res["condition_a"] and res["condition_b"] and res["linearize_fused_bit_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
