#!/usr/bin/env python3
"""Reverse-mode rollout: what the backward sweep costs next to the forward rollout that records its Jacobians.

Workload (default): Ant, fp32, B = 4096, H = 20 -- the record is H B nx (nx + nu) 4 bytes = 8.7 GB of device memory.
Method: both calls are enqueued on one stream between hipEvents (torch.cuda.Event), after a warm-up of each; `--reps` repetitions, alternating
the two, the median of each is reported.  Printed:
  (a) ms per step of the recording rollout (dojo_rollout_record_dev: the differentiable step of bench.py, H times, Jacobians kept),
  (b) ms per step of the reverse sweep (dojo_rollout_adjoint_dev, one launch) and the bytes of DZ + DU it streams over that time,
  (c) the ratio (b) / (a); the condition is (c) <= 0.25, and the tool exits with status 1 when it is missed.
The bytes are the algorithm's: every Jacobian entry of a step that did not fail is read once; G, Z and the outputs are left out (< 1 %).
A last line is the same as JSON.  Needs a GPU: there is no fallback.

    python tools/adjoint_bench.py [--batch 4096] [--steps 20] [--dtype f32] [--reps 7] [--config 3] [--cot-space state|tangent]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dojo.jl_amd", "host"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--config", type=int, default=3, help="BASELINE.md configuration (3 = Ant)")
    ap.add_argument("--cot-space", default="state", choices=["state", "tangent"])
    a = ap.parse_args()

    import numpy as np
    import torch                      # (first: torch brings the GPU up, INTEGRATION.md "Using the library next to PyTorch")
    if not torch.cuda.is_available():
        raise SystemExit("adjoint_bench: no GPU")
    torch.cuda.init()
    import dojo_amd as d
    from dojo_amd import api

    spec = d.baseline_config(a.config)
    B, H, nx, nu, nz = a.batch, a.steps, spec.nx, spec.nu, spec.nz
    gm = api.BatchedMechanism(spec, B, dtype=a.dtype)
    tdt = torch.float32 if a.dtype == "f32" else torch.float64
    w = 4 if a.dtype == "f32" else 8
    z0, u = d.synthetic_inputs(spec, B)
    rng = np.random.default_rng(1)
    U = np.stack([u * rng.uniform(0.5, 1.0) for _ in range(H)])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x.astype(gm.np_dtype))).cuda()
    z0d, Ud = dev(z0), dev(U)
    Z = torch.empty((H, B, nz), dtype=tdt, device="cuda"); st = torch.empty((H, B), dtype=torch.int32, device="cuda")
    DZ = torch.empty((H, B, nx, nx), dtype=tdt, device="cuda"); DU = torch.empty((H, B, max(nu, 1), nx), dtype=tdt, device="cuda")
    cs = 1 if a.cot_space == "state" else 0
    G = dev(rng.standard_normal((H, B, nz if cs else nx)))
    gU = torch.empty((H, B, max(nu, 1)), dtype=tdt, device="cuda"); gz = torch.empty((B, nx), dtype=tdt, device="cuda")
    stream = api.torch_stream()
    L = api.lib()

    def forward():
        api._chk(L.dojo_rollout_record_dev(gm.h, api.addr(z0d), api.addr(Ud), H, api.addr(Z), api.addr(st), api.addr(DZ), api.addr(DU), stream))

    def backward():
        api._chk(L.dojo_rollout_adjoint_dev(gm.h, H, api.addr(DZ), api.addr(DU), api.addr(G), cs, api.addr(Z), api.addr(st), api.addr(gU), api.addr(gz), stream))

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    forward(); backward(); torch.cuda.synchronize()          # warm-up: code objects, workspaces, the streams of the environment groups
    tf, tb = [], []
    for _ in range(a.reps):
        tf.append(timed(forward)); tb.append(timed(backward))
    ok_steps = int((st == 0).sum().item())
    finite = bool(torch.isfinite(gz).all().item() and torch.isfinite(gU).all().item())
    bytes_read = ok_steps * nx * (nx + nu) * w
    f_ms, b_ms = statistics.median(tf) / H, statistics.median(tb) / H
    res = {"tool": "adjoint_bench", "mechanism": spec.name, "dtype": a.dtype, "batch": B, "steps": H, "reps": a.reps, "cot_space": a.cot_space,
           "record_bytes": H * B * nx * (nx + nu) * w, "solved_env_steps": ok_steps, "env_steps": H * B, "outputs_finite": finite,
           "forward_record_ms_per_step": round(f_ms, 4), "forward_ms_per_step_runs": [round(t / H, 4) for t in tf],
           "adjoint_ms_per_step": round(b_ms, 4), "adjoint_ms_per_step_runs": [round(t / H, 4) for t in tb],
           "adjoint_jacobian_bytes": bytes_read, "adjoint_tb_per_s": round(bytes_read / (statistics.median(tb) * 1e-3) / 1e12, 3),
           "ratio_adjoint_over_forward": round(b_ms / f_ms, 4), "condition_ratio_le": 0.25}
    res["condition_met"] = bool(res["ratio_adjoint_over_forward"] <= 0.25)
    print("%s %s  B = %d  H = %d   record %.2f GB   %d of %d environment-steps solved" % (spec.name, a.dtype, B, H, res["record_bytes"] / 1e9, ok_steps, H * B))
    print("(a) recording rollout   %8.3f ms per step   (runs: %s)" % (f_ms, " ".join("%.3f" % (t / H) for t in tf)))
    print("(b) reverse sweep       %8.3f ms per step   (runs: %s)   %.2f TB/s of DZ + DU" % (b_ms, " ".join("%.3f" % (t / H) for t in tb), res["adjoint_tb_per_s"]))
    print("(c) (b) / (a)           %8.3f              condition <= 0.25: %s" % (res["ratio_adjoint_over_forward"], "met" if res["condition_met"] else "MISSED"))
    print(json.dumps(res))
    gm.close()
    return 0 if res["condition_met"] and finite else 1


if __name__ == "__main__":
    sys.exit(main())
