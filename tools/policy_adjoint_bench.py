#!/usr/bin/env python3
"""Reverse mode through a closed-loop rollout: what the policy-gradient sweep costs next to the forward rollout that records its Jacobians.

Workload (default): Ant, fp32, B = 4096, H = 20, one policy per environment (per_env = 1), contact_forces = 0 -- the record is
H B nx (nx + nu) 4 bytes = 8.7 GB of device memory, the observation Jacobians (H + 1) B 2nu 24 8 bytes = 0.46 GB.
Method: the calls are enqueued on one stream between hipEvents (torch.cuda.Event), after a warm-up of each; `--reps` repetitions, alternating
the three, the median of each is reported.  Printed:
  (a) ms per step of the recording closed-loop rollout (dojo_rollout_policy_record_dev),
  (b) ms per step of the closed-loop sweep INCLUDING its observation-Jacobian prepass (dojo_rollout_policy_adjoint_dev with M = NULL: two
      launches, three with --shared) and the bytes of DZ + DU + M it streams over that time,
  (c) ms per step of the open-loop sweep (dojo_rollout_adjoint_dev) on the same record, for information,
  (b) / (a), whose condition is <= 0.25 (the tool exits with status 1 when it is missed), and (b) / (c) without a condition.
A last line is the same as JSON.  Needs a GPU: there is no fallback.

    python tools/policy_adjoint_bench.py [--batch 4096] [--steps 20] [--dtype f32] [--reps 7] [--config 3] [--shared]
"""
import argparse
import ctypes as C
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
    ap.add_argument("--shared", action="store_true", help="one policy for all environments (per_env = 0: the sweep is followed by the reduction over the batch)")
    a = ap.parse_args()

    import numpy as np
    import torch                      # (first: torch brings the GPU up, INTEGRATION.md "Using the library next to PyTorch")
    if not torch.cuda.is_available():
        raise SystemExit("policy_adjoint_bench: no GPU")
    torch.cuda.init()
    import dojo_amd as d
    from dojo_amd import api

    spec = d.baseline_config(a.config)
    B, H, nx, nu, nz = a.batch, a.steps, spec.nx, spec.nu, spec.nz
    nobs = 2 * nu
    act_off = 6 if nu > 6 else 0      # (the floating base of Ant / Atlas is not driven)
    na = nu - act_off
    gm = api.BatchedMechanism(spec, B, dtype=a.dtype)
    tdt = torch.float32 if a.dtype == "f32" else torch.float64
    w = 4 if a.dtype == "f32" else 8
    z0, _ = d.synthetic_inputs(spec, B)
    rng = np.random.default_rng(1)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x.astype(gm.np_dtype))).cuda()
    Bw = 1 if a.shared else B
    U_ff = np.zeros((H, B, nu)); U_ff[:, :, act_off:] = 0.2 * rng.standard_normal((H, B, na))
    z0d, Wd, bd = dev(z0), dev(0.1 * rng.standard_normal((Bw, na, nobs))), dev(0.1 * rng.standard_normal((Bw, na)))
    md, sd, Ud = dev(0.1 * rng.standard_normal(nobs)), dev(rng.uniform(0.5, 1.5, nobs)), dev(U_ff)
    pol = api.DojoPolicy(Wd.data_ptr(), bd.data_ptr(), md.data_ptr(), sd.data_ptr(), Ud.data_ptr(), 0 if a.shared else 1, act_off, na, 0, 0, 0)
    e = lambda *shape, dt=tdt: torch.empty(shape, dtype=dt, device="cuda")
    Z, OBS, U, st = e(H, B, nz), e(H + 1, B, nobs), e(H, B, nu), e(H, B, dt=torch.int32)
    DZ, DU = e(H, B, nx, nx), e(H, B, nu, nx)
    G, Gu, Go = dev(rng.standard_normal((H, B, nz))), dev(rng.standard_normal((H, B, nu))), dev(rng.standard_normal((H + 1, B, nobs)))
    gW, gb, gU, gz = e(Bw, na, nobs), e(Bw, na), e(H, B, nu), e(B, nx)
    gU2, gz2 = e(H, B, nu), e(B, nx)
    adj = api.DojoPolicyAdjoint(DZ.data_ptr(), DU.data_ptr(), OBS.data_ptr(), st.data_ptr(), z0d.data_ptr(), Z.data_ptr(), None, G.data_ptr(), Gu.data_ptr(),
                                Go.data_ptr(), gW.data_ptr(), gb.data_ptr(), gU.data_ptr(), gz.data_ptr(), 1, 0)
    stream = api.torch_stream()
    L = api.lib()

    def forward():
        api._chk(L.dojo_rollout_policy_record_dev(gm.h, api.addr(z0d), C.byref(pol), H, api.addr(Z), api.addr(OBS), api.addr(U), api.addr(st), api.addr(DZ), api.addr(DU), stream))

    def backward():
        api._chk(L.dojo_rollout_policy_adjoint_dev(gm.h, C.byref(pol), H, C.byref(adj), stream))

    def open_loop():
        api._chk(L.dojo_rollout_adjoint_dev(gm.h, H, api.addr(DZ), api.addr(DU), api.addr(G), 1, api.addr(Z), api.addr(st), api.addr(gU2), api.addr(gz2), stream))

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    forward(); backward(); open_loop(); torch.cuda.synchronize()          # warm-up: code objects, workspaces, the streams of the environment groups
    tf, tb, to = [], [], []
    for _ in range(a.reps):
        tf.append(timed(forward)); tb.append(timed(backward)); to.append(timed(open_loop))
    ok_steps = int((st == 0).sum().item())
    finite = bool(all(torch.isfinite(t).all().item() for t in (gW, gb, gU, gz)))
    m_bytes = (H + 1) * B * nobs * 24 * 8
    bytes_read = ok_steps * nx * (nx + nu) * w + m_bytes
    f_ms, b_ms, o_ms = statistics.median(tf) / H, statistics.median(tb) / H, statistics.median(to) / H
    res = {"tool": "policy_adjoint_bench", "mechanism": spec.name, "dtype": a.dtype, "batch": B, "steps": H, "reps": a.reps, "per_env": 0 if a.shared else 1,
           "na": na, "nobs": nobs, "record_bytes": H * B * nx * (nx + nu) * w, "observation_jacobian_bytes": m_bytes, "solved_env_steps": ok_steps,
           "env_steps": H * B, "outputs_finite": finite,
           "forward_record_ms_per_step": round(f_ms, 4), "forward_ms_per_step_runs": [round(t / H, 4) for t in tf],
           "policy_adjoint_ms_per_step": round(b_ms, 4), "policy_adjoint_ms_per_step_runs": [round(t / H, 4) for t in tb],
           "open_loop_adjoint_ms_per_step": round(o_ms, 4), "open_loop_adjoint_ms_per_step_runs": [round(t / H, 4) for t in to],
           "policy_adjoint_bytes": bytes_read, "policy_adjoint_tb_per_s": round(bytes_read / (statistics.median(tb) * 1e-3) / 1e12, 3),
           "ratio_policy_adjoint_over_forward": round(b_ms / f_ms, 4), "ratio_policy_adjoint_over_open_loop": round(b_ms / o_ms, 3), "condition_ratio_le": 0.25}
    res["condition_met"] = bool(res["ratio_policy_adjoint_over_forward"] <= 0.25)
    runs = lambda t: " ".join("%.3f" % (x / H) for x in t)
    print("%s %s  B = %d  H = %d  na = %d  nobs = %d  per_env = %d   record %.2f GB + M %.2f GB   %d of %d environment-steps solved"
          % (spec.name, a.dtype, B, H, na, nobs, res["per_env"], res["record_bytes"] / 1e9, m_bytes / 1e9, ok_steps, H * B))
    print("(a) recording closed-loop rollout   %8.3f ms per step   (runs: %s)" % (f_ms, runs(tf)))
    print("(b) closed-loop sweep + M prepass   %8.3f ms per step   (runs: %s)   %.2f TB/s of DZ + DU + M" % (b_ms, runs(tb), res["policy_adjoint_tb_per_s"]))
    print("(c) open-loop sweep, same record    %8.3f ms per step   (runs: %s)" % (o_ms, runs(to)))
    print("    (b) / (a)                       %8.3f              condition <= 0.25: %s" % (res["ratio_policy_adjoint_over_forward"], "met" if res["condition_met"] else "MISSED"))
    print("    (b) / (c)                       %8.3f" % res["ratio_policy_adjoint_over_open_loop"])
    print(json.dumps(res))
    gm.close()
    return 0 if res["condition_met"] and finite else 1


if __name__ == "__main__":
    sys.exit(main())
