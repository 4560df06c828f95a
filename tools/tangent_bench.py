#!/usr/bin/env python3
"""Forward-mode rollout: what the multi-tangent sweep costs next to the rollout that records its Jacobians and next to the reverse sweep over the same record.

Workload (default): Ant, fp32, B = 4096, H = 20 -- the record of tools/adjoint_bench.py plus the contact-data columns (dojo_rollout_data_record_dev).
Method: every call is enqueued on one stream between hipEvents (torch.cuda.Event), after a warm-up of each; `--reps` repetitions, alternating the five, the
median of each is reported.  Printed, in ms per step and -- for the sweeps -- TB/s of the record bytes they read (DZ + DU of every step that did not fail, once
per sweep, however many tangents; tangents, G and outputs are left out):
  (a) the recording rollout (dojo_rollout_data_record_dev),
  (b) the reverse sweep over DZ + DU (dojo_rollout_adjoint_dev, one launch): the project's measured bandwidth yardstick,
  (c) the tangent sweep (dojo_rollout_tangent_dev, dz0 and dU given: the same DZ + DU) at T = 1,  (d) at T = 4,  (e) at T = 8.
Conditions (the tool exits with status 1 when one is missed): (d) <= 0.25 (a);  (d) < 4 (c) by more than four times the run-to-run spread (max - min) of (c).
(c) / (b) is reported, not gated.  A last line is the same as JSON.  Needs a GPU: there is no fallback.

    python tools/tangent_bench.py [--batch 4096] [--steps 20] [--dtype f32] [--reps 7] [--config 3]
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
    a = ap.parse_args()

    import numpy as np
    import torch                      # (first: torch brings the GPU up, INTEGRATION.md "Using the library next to PyTorch")
    if not torch.cuda.is_available():
        raise SystemExit("tangent_bench: no GPU")
    torch.cuda.init()
    import dojo_amd as d
    from dojo_amd import api

    spec = d.baseline_config(a.config)
    B, H, nx, nu, nz, nth = a.batch, a.steps, spec.nx, spec.nu, spec.nz, 5 * len(spec.contacts)
    gm = api.BatchedMechanism(spec, B, dtype=a.dtype)
    tdt = torch.float32 if a.dtype == "f32" else torch.float64
    w = 4 if a.dtype == "f32" else 8
    z0, u = d.synthetic_inputs(spec, B)
    rng = np.random.default_rng(1)
    U = np.stack([u * rng.uniform(0.5, 1.0) for _ in range(H)])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x.astype(gm.np_dtype))).cuda()
    empty = lambda *shape: torch.empty(shape, dtype=tdt, device="cuda")
    z0d, Ud = dev(z0), dev(U)
    Z = empty(H, B, nz); st = torch.empty((H, B), dtype=torch.int32, device="cuda")
    DZ, DU, DC = empty(H, B, nx, nx), empty(H, B, max(nu, 1), nx), (empty(H, B, nth, nx) if nth else None)
    G = dev(rng.standard_normal((H, B, nz)))
    gU, gz = empty(H, B, max(nu, 1)), empty(B, nx)
    TS = (1, 4, 8)
    dz0 = torch.randn((B, max(TS), nx), dtype=tdt, device="cuda")           # [B][T][nx] of a smaller T is not a slice of it: one buffer per T
    tan = {T: (dz0[:, :T].contiguous(), torch.randn((H, B, T, max(nu, 1)), dtype=tdt, device="cuda"), empty(H, B, T, nz)) for T in TS}
    stream = api.torch_stream()
    L = api.lib()

    def forward():
        api._chk(L.dojo_rollout_data_record_dev(gm.h, api.addr(z0d), api.addr(Ud), H, api.addr(Z), api.addr(st), api.addr(DZ), api.addr(DU), api.addr(DC), stream))

    def backward():
        api._chk(L.dojo_rollout_adjoint_dev(gm.h, H, api.addr(DZ), api.addr(DU), api.addr(G), 1, api.addr(Z), api.addr(st), api.addr(gU), api.addr(gz), stream))

    def tangent(T):
        d0, dU, out = tan[T]
        return lambda: api._chk(L.dojo_rollout_tangent_dev(gm.h, H, T, api.addr(DZ), api.addr(DU), None, api.addr(d0), api.addr(dU) if nu else None, None, 1, api.addr(Z), api.addr(st), api.addr(out), stream))

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    calls = [("a", forward), ("b", backward)] + [(k, tangent(T)) for k, T in zip("cde", TS)]
    for _, f in calls:                                                      # warm-up: code objects, workspaces, the streams of the environment groups
        f()
    torch.cuda.synchronize()
    runs = {k: [] for k, _ in calls}
    for _ in range(a.reps):
        for k, f in calls:
            runs[k].append(timed(f))
    ok_steps = int((st == 0).sum().item())
    finite = bool(torch.isfinite(gz).all().item() and all(torch.isfinite(tan[T][2]).all().item() for T in TS))
    bytes_read = ok_steps * nx * (nx + nu) * w
    ms = {k: statistics.median(v) / H for k, v in runs.items()}
    tbs = {k: bytes_read / (statistics.median(runs[k]) * 1e-3) / 1e12 for k in "bcde"}
    spread_c = (max(runs["c"]) - min(runs["c"])) / H
    res = {"tool": "tangent_bench", "mechanism": spec.name, "dtype": a.dtype, "batch": B, "steps": H, "reps": a.reps,
           "record_bytes": H * B * nx * (nx + nu + nth) * w, "sweep_jacobian_bytes": bytes_read, "solved_env_steps": ok_steps, "env_steps": H * B, "outputs_finite": finite,
           "ms_per_step": {k: round(v, 4) for k, v in ms.items()}, "ms_per_step_runs": {k: [round(t / H, 4) for t in v] for k, v in runs.items()},
           "tb_per_s": {k: round(v, 3) for k, v in tbs.items()}, "spread_c_ms_per_step": round(spread_c, 4),
           "ratio_d_over_a": round(ms["d"] / ms["a"], 4), "ratio_d_over_c": round(ms["d"] / ms["c"], 4), "ratio_e_over_c": round(ms["e"] / ms["c"], 4),
           "ratio_c_over_b": round(ms["c"] / ms["b"], 4)}
    res["condition_d_le_quarter_a"] = bool(ms["d"] <= 0.25 * ms["a"])
    res["condition_d_lt_4c"] = bool(4 * ms["c"] - ms["d"] > 4 * spread_c)
    names = {"a": "recording rollout (with DC)", "b": "reverse sweep, DZ + DU    ", "c": "tangent sweep, T = 1      ", "d": "tangent sweep, T = 4      ", "e": "tangent sweep, T = 8      "}
    print("%s %s  B = %d  H = %d   record %.2f GB   %d of %d environment-steps solved" % (spec.name, a.dtype, B, H, res["record_bytes"] / 1e9, ok_steps, H * B))
    for k, _ in calls:
        print("(%s) %s %8.3f ms per step   (runs: %s)%s" % (k, names[k], ms[k], " ".join("%.3f" % (t / H) for t in runs[k]), "" if k == "a" else "   %.2f TB/s of DZ + DU" % tbs[k]))
    print("(d) / (a) = %.3f   condition <= 0.25: %s" % (res["ratio_d_over_a"], "met" if res["condition_d_le_quarter_a"] else "MISSED"))
    print("(d) / (c) = %.3f, (e) / (c) = %.3f   condition (d) < 4 (c) by more than 4 x the spread of (c) (%.4f ms): %s"
          % (res["ratio_d_over_c"], res["ratio_e_over_c"], spread_c, "met" if res["condition_d_lt_4c"] else "MISSED"))
    print("(c) / (b) = %.3f   (reported, not gated)" % res["ratio_c_over_b"])
    print(json.dumps(res))
    gm.close()
    return 0 if res["condition_d_le_quarter_a"] and res["condition_d_lt_4c"] and finite else 1


if __name__ == "__main__":
    sys.exit(main())
