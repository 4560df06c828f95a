#!/usr/bin/env python3
"""Closed-loop rollout: what evaluating the policy on the device between the steps costs next to the open-loop rollout of the same trajectories.

Workload (default): Ant, fp32, B = 4096, H = 60, the library's default (joined-at-end) rollout groups, after a warm-up rollout.
  (A) dojo_rollout_dev, open loop, fed with the U_out a closed-loop run recorded: the same trajectories, hence the same solver work
  (B) dojo_rollout_policy_dev with one policy per environment, OBS and U_out recorded
Method: every call is enqueued on one stream between device events (torch.cuda.Event) and the device is synchronised after it; order A B B A,
`--rounds` rounds; the condition is mean(B) / mean(A) <= 1.10, and the tool exits with status 1 when it is missed.
For information only: env-steps/s of the stepwise loop of examples/ant_ars_device.py (dojo_observe_dev, torch, dojo_step_minimal_dev per step) at the same
B and H -- the AntARS environment's mechanism (body contacts included), wall clock around a synchronised rollout.
A last line is the same as JSON.  Needs a GPU: there is no fallback.

    python tools/policy_bench.py [--batch 4096] [--steps 60] [--dtype f32] [--rounds 2] [--config 3] [--no-stepwise]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dojo.jl_amd", "host"))
sys.path.insert(0, os.path.join(ROOT, "examples"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--config", type=int, default=3, help="BASELINE.md configuration (3 = Ant)")
    ap.add_argument("--no-stepwise", action="store_true", help="skip the stepwise loop of examples/ant_ars_device.py")
    a = ap.parse_args()

    import numpy as np
    import torch                      # (first: torch brings the GPU up, INTEGRATION.md "Using the library next to PyTorch")
    if not torch.cuda.is_available():
        raise SystemExit("policy_bench: no GPU")
    torch.cuda.init()
    import dojo_amd as d
    from dojo_amd import api

    spec = d.baseline_config(a.config)
    B, H, nu, nz = a.batch, a.steps, spec.nu, spec.nz
    act_off = 6 if nu > 6 else 0
    na, nobs = nu - act_off, 2 * nu + len(spec.contacts)
    gm = api.BatchedMechanism(spec, B, dtype=a.dtype)
    tdt = torch.float32 if a.dtype == "f32" else torch.float64
    rng = np.random.default_rng(1)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(gm.np_dtype))).cuda()
    z0 = dev(d.synthetic_inputs(spec, B)[0])
    W = dev(0.1 * rng.standard_normal((B, na, nobs))); mean = dev(0.1 * rng.standard_normal(nobs)); scale = dev(rng.uniform(0.5, 1.5, nobs))
    Uff = np.zeros((H, B, nu)); Uff[:, :, act_off:] = 0.2 * rng.standard_normal((H, B, na)); Uff = dev(Uff)
    Z = torch.empty((H, B, nz), dtype=tdt, device="cuda"); st = torch.empty((H, B), dtype=torch.int32, device="cuda")
    OBS = torch.empty((H + 1, B, nobs), dtype=tdt, device="cuda"); U = torch.empty((H, B, nu), dtype=tdt, device="cuda")
    pol = api.DojoPolicy(W.data_ptr(), None, mean.data_ptr(), scale.data_ptr(), Uff.data_ptr(), 1, act_off, na, 1, 0, 0)
    stream = api.torch_stream()
    L = api.lib()

    def closed():
        api._chk(L.dojo_rollout_policy_dev(gm.h, api.addr(z0), C.byref(pol), H, api.addr(Z), api.addr(OBS), api.addr(U), api.addr(st), stream))

    closed(); torch.cuda.synchronize()                          # warm-up: code objects, workspaces, the streams of the environment groups
    Urec = U.clone(); solved = int((st == 0).sum().item())

    def open_loop():
        api._chk(L.dojo_rollout_dev(gm.h, api.addr(z0), api.addr(Urec), H, api.addr(Z), api.addr(st), stream))

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); e1.synchronize(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    open_loop(); torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(timed(open_loop)); tb.append(timed(closed)); tb.append(timed(closed)); ta.append(timed(open_loop))
    same = bool(torch.equal(U, Urec))
    ma, mb = statistics.mean(ta), statistics.mean(tb)
    res = {"tool": "policy_bench", "mechanism": spec.name, "dtype": a.dtype, "batch": B, "steps": H, "rounds": a.rounds, "nobs": nobs, "na": na,
           "solved_env_steps": solved, "env_steps": H * B, "controls_reproduced": same,
           "open_loop_ms": round(ma, 3), "open_loop_ms_runs": [round(t, 3) for t in ta], "closed_loop_ms": round(mb, 3), "closed_loop_ms_runs": [round(t, 3) for t in tb],
           "open_loop_env_steps_per_s": round(H * B / (ma * 1e-3)), "closed_loop_env_steps_per_s": round(H * B / (mb * 1e-3)),
           "ratio_closed_over_open": round(mb / ma, 4), "condition_ratio_le": 1.10}
    res["condition_met"] = bool(res["ratio_closed_over_open"] <= 1.10)
    print("%s %s  B = %d  H = %d  nobs = %d  na = %d   %d of %d environment-steps solved" % (spec.name, a.dtype, B, H, nobs, na, solved, H * B))
    print("(A) open loop, recorded controls   %9.3f ms per rollout  %9.0f env-steps/s   (runs: %s)" % (ma, res["open_loop_env_steps_per_s"], " ".join("%.3f" % t for t in ta)))
    print("(B) closed loop, policy on device  %9.3f ms per rollout  %9.0f env-steps/s   (runs: %s)" % (mb, res["closed_loop_env_steps_per_s"], " ".join("%.3f" % t for t in tb)))
    print("(B) / (A)                          %9.3f                condition <= 1.10: %s" % (res["ratio_closed_over_open"], "met" if res["condition_met"] else "MISSED"))
    gm.close()
    if not a.no_stepwise:
        import ant_ars_device as ars
        from dojo_amd.envs import BatchedEnvironment
        env = BatchedEnvironment("ant_ars", B, dtype=a.dtype)
        theta = (0.1 * torch.randn(B, env.spec.nu - env.n_unactuated, env.nobs, device=env.device)).to(env.torch_dtype)
        norm = ars.Normalizer(env.nobs, env.torch_dtype, env.device)
        rates = []
        for _ in range(2):                                      # (the first run warms up)
            torch.cuda.synchronize(); t0 = time.time()
            ars.rollout_policy(theta, env, norm, H)
            torch.cuda.synchronize(); rates.append(B * H / (time.time() - t0))
        env.close()
        res["stepwise_example_env_steps_per_s"] = round(rates[-1])
        print("(for information) stepwise loop of examples/ant_ars_device.py, AntARS mechanism: %9.0f env-steps/s" % rates[-1])
    print(json.dumps(res))
    return 0 if res["condition_met"] and same else 1


if __name__ == "__main__":
    sys.exit(main())
