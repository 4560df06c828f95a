#!/usr/bin/env python3
"""Contact-data gradients through a rollout: what the contact-data columns cost the recording rollout, and what the contact-data sweep costs next
to the open-loop sweep over the same record.

Workload (default): Ant, fp32, B = 4096, H = 20 -- the record is H B nx (nx + nu + 5 Nc) 4 bytes = 9.7 GB of device memory.
Method: the five calls are enqueued on one stream between hipEvents (torch.cuda.Event), after one warm-up of each; `--reps` repetitions in one
process, the five in a seeded random order that changes from one repetition to the next (a sweep is 10-20 % faster behind a rollout than behind another sweep), the median of each is reported.  Printed, in ms per step:
  (a) dojo_rollout_record_dev        the recording rollout (step + IFT kernel per step and environment group),
  (b) dojo_rollout_data_record_dev   the same plus one contact-data IFT launch per step and group; (b) / (a) as measured, no target,
  (c) dojo_rollout_adjoint_dev       the open-loop sweep, with the bytes of DZ + DU it streams and the rate,
  (d) dojo_rollout_data_adjoint_dev  the contact-data sweep (gtheta_env, gtheta and gz: the sweep and the reduction over the batch), with the bytes
                                     of DZ + DC it streams and the rate; (d)'s rate over (c)'s from the same run,
  (e) the same without gtheta        the sweep alone (no workspace, no reduction launch): what the shared sum costs is (d) - (e).
The bytes are the algorithm's: every Jacobian entry of a step that did not fail is read once; G, Z and the outputs are left out (< 1 %).
A last line is the same as JSON.  Needs a GPU: there is no fallback.

    python tools/data_adjoint_bench.py [--batch 4096] [--steps 20] [--dtype f32] [--reps 7] [--config 3] [--cot-space state|tangent]
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
        raise SystemExit("data_adjoint_bench: no GPU")
    torch.cuda.init()
    import dojo_amd as d
    from dojo_amd import api

    spec = d.baseline_config(a.config)
    B, H, nx, nu, nz, nth = a.batch, a.steps, spec.nx, spec.nu, spec.nz, 5 * len(spec.contacts)
    if nth == 0:
        raise SystemExit("data_adjoint_bench: the mechanism has no contacts")
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
    DC = torch.empty((H, B, nth, nx), dtype=tdt, device="cuda")
    cs = 1 if a.cot_space == "state" else 0
    G = dev(rng.standard_normal((H, B, nz if cs else nx)))
    gU = torch.empty((H, B, max(nu, 1)), dtype=tdt, device="cuda"); gz = torch.empty((B, nx), dtype=tdt, device="cuda")
    gte = torch.empty((B, nth), dtype=tdt, device="cuda"); gt = torch.empty((nth,), dtype=tdt, device="cuda"); gz2 = torch.empty((B, nx), dtype=tdt, device="cuda")
    stream = api.torch_stream()
    L = api.lib()

    def record():
        api._chk(L.dojo_rollout_record_dev(gm.h, api.addr(z0d), api.addr(Ud), H, api.addr(Z), api.addr(st), api.addr(DZ), api.addr(DU), stream))

    def data_record():
        api._chk(L.dojo_rollout_data_record_dev(gm.h, api.addr(z0d), api.addr(Ud), H, api.addr(Z), api.addr(st), api.addr(DZ), api.addr(DU), api.addr(DC), stream))

    def sweep():
        api._chk(L.dojo_rollout_adjoint_dev(gm.h, H, api.addr(DZ), api.addr(DU), api.addr(G), cs, api.addr(Z), api.addr(st), api.addr(gU), api.addr(gz), stream))

    def data_sweep():
        api._chk(L.dojo_rollout_data_adjoint_dev(gm.h, H, api.addr(DZ), api.addr(DC), api.addr(G), cs, api.addr(Z), api.addr(st), api.addr(gte), api.addr(gt), api.addr(gz2), stream))

    def data_sweep_env():
        api._chk(L.dojo_rollout_data_adjoint_dev(gm.h, H, api.addr(DZ), api.addr(DC), api.addr(G), cs, api.addr(Z), api.addr(st), api.addr(gte), None, api.addr(gz2), stream))

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    calls = (record, data_record, sweep, data_sweep, data_sweep_env)
    for f in calls:                                           # warm-up: code objects, workspaces, the streams of the environment groups
        f()
    torch.cuda.synchronize()
    t = [[] for _ in calls]
    order = np.random.default_rng(2)
    for _ in range(a.reps):                                   # a fresh seeded order every time: what a call follows (a long rollout, another sweep) moves a sweep's time by 10-20 %
        for i in order.permutation(len(calls)):
            t[i].append(timed(calls[i]))
    ok_steps = int((st == 0).sum().item())
    finite = bool(all(torch.isfinite(x).all().item() for x in (gz, gU, gte, gt, gz2)))
    same_gz = bool(torch.equal(gz, gz2))                      # (both sweeps push the same lambda through the same columns of DZ)
    med = [statistics.median(x) for x in t]
    bytes_c, bytes_d = ok_steps * nx * (nx + nu) * w, ok_steps * nx * (nx + nth) * w
    tb_c, tb_d = bytes_c / (med[2] * 1e-3) / 1e12, bytes_d / (med[3] * 1e-3) / 1e12
    runs = lambda x: " ".join("%.3f" % (v / H) for v in x)
    res = {"tool": "data_adjoint_bench", "mechanism": spec.name, "dtype": a.dtype, "batch": B, "steps": H, "reps": a.reps, "cot_space": a.cot_space,
           "record_bytes": H * B * nx * (nx + nu + nth) * w, "solved_env_steps": ok_steps, "env_steps": H * B, "outputs_finite": finite, "gz_of_both_sweeps_equal": same_gz,
           "record_ms_per_step": round(med[0] / H, 4), "record_ms_per_step_runs": [round(v / H, 4) for v in t[0]],
           "data_record_ms_per_step": round(med[1] / H, 4), "data_record_ms_per_step_runs": [round(v / H, 4) for v in t[1]],
           "ratio_data_record_over_record": round(med[1] / med[0], 4),
           "adjoint_ms_per_step": round(med[2] / H, 4), "adjoint_ms_per_step_runs": [round(v / H, 4) for v in t[2]], "adjoint_jacobian_bytes": bytes_c, "adjoint_tb_per_s": round(tb_c, 3),
           "data_adjoint_ms_per_step": round(med[3] / H, 4), "data_adjoint_ms_per_step_runs": [round(v / H, 4) for v in t[3]], "data_adjoint_jacobian_bytes": bytes_d,
           "data_adjoint_tb_per_s": round(tb_d, 3), "ratio_data_adjoint_rate_over_adjoint_rate": round(tb_d / tb_c, 4),
           "data_adjoint_without_sum_ms_per_step": round(med[4] / H, 4), "data_adjoint_without_sum_ms_per_step_runs": [round(v / H, 4) for v in t[4]]}
    print("%s %s  B = %d  H = %d   record %.2f GB   %d of %d environment-steps solved" % (spec.name, a.dtype, B, H, res["record_bytes"] / 1e9, ok_steps, H * B))
    print("(a) recording rollout            %8.3f ms per step   (runs: %s)" % (med[0] / H, runs(t[0])))
    print("(b) ... with contact-data columns %7.3f ms per step   (runs: %s)   (b) / (a) = %.3f" % (med[1] / H, runs(t[1]), med[1] / med[0]))
    print("(c) open-loop sweep              %8.3f ms per step   (runs: %s)   %.2f TB/s of DZ + DU" % (med[2] / H, runs(t[2]), tb_c))
    print("(d) contact-data sweep           %8.3f ms per step   (runs: %s)   %.2f TB/s of DZ + DC   (d) / (c) rate = %.3f" % (med[3] / H, runs(t[3]), tb_d, tb_d / tb_c))
    print("(e) ... without the shared sum   %8.3f ms per step   (runs: %s)   %.2f TB/s" % (med[4] / H, runs(t[4]), bytes_d / (med[4] * 1e-3) / 1e12))
    print(json.dumps(res))
    gm.close()
    return 0 if finite and same_gz else 1


if __name__ == "__main__":
    sys.exit(main())
