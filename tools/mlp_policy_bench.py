#!/usr/bin/env python3
"""Closed-loop rollouts with a tanh network policy: what the controller costs next to the open-loop rollout of the same trajectories, and what the
reverse sweep through it costs next to the forward rollout that records its Jacobians.  The methods are those of tools/policy_bench.py and
tools/policy_adjoint_bench.py: every call is enqueued on one stream between device events (torch.cuda.Event), after a warm-up of each, the legs
alternating in one process.

Workload (default): Ant, fp32, B = 4096, widths [28, 64, 64, 8] (two hidden layers of 64, contact_forces = 0).  The SHARED policy (per_env = 0) is the
asserted case; one policy per environment (per_env = 1) and the affine policy are reported for information.

Forward, H = --steps (60), order A B C D D C B A per round, means:
  (A) dojo_rollout_dev, open loop, fed with the U_out the shared network recorded: the same trajectories, hence the same solver work
  (B) dojo_rollout_mlp_dev, shared network, OBS, U_out and ACT recorded          condition: mean(B) / mean(A) <= 1.10
  (C) dojo_rollout_mlp_dev, one network per environment
  (D) dojo_rollout_policy_dev, affine, one policy per environment
Reverse, H = --rsteps (20), the legs alternating, medians, per step:
  (a) dojo_rollout_mlp_record_dev, shared network: the recording rollout
  (b) dojo_rollout_mlp_adjoint_dev with M = NULL, shared: the observation-Jacobian prepass, the sweep and the reduction      condition: (b) / (a) <= 0.25
  (c) the same with one network per environment (no reduction), on the same record
  (d) dojo_rollout_policy_adjoint_dev, affine, shared and (e) one policy per environment, on the same record (DZ, DU, OBS, Z)
The tool exits with status 1 when a condition is missed.  A last line is the same as JSON.  Needs a GPU: there is no fallback.

    python tools/mlp_policy_bench.py [--batch 4096] [--steps 60] [--rsteps 20] [--dtype f32] [--rounds 2] [--reps 7] [--hidden 64 64] [--config 3]
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
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rsteps", type=int, default=20)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--hidden", type=int, nargs="*", default=[64, 64])
    ap.add_argument("--config", type=int, default=3, help="BASELINE.md configuration (3 = Ant)")
    a = ap.parse_args()

    import numpy as np
    import torch                      # (first: torch brings the GPU up, INTEGRATION.md "Using the library next to PyTorch")
    if not torch.cuda.is_available():
        raise SystemExit("mlp_policy_bench: no GPU")
    torch.cuda.init()
    import dojo_amd as d
    from dojo_amd import api

    spec = d.baseline_config(a.config)
    B, nx, nu, nz = a.batch, spec.nx, spec.nu, spec.nz
    act_off = 6 if nu > 6 else 0      # (the floating base of Ant / Atlas is not driven)
    na, nobs = nu - act_off, 2 * nu
    widths = [nobs] + list(a.hidden) + [na]
    Pn, nh = api.mlp_sizes(widths)
    gm = api.BatchedMechanism(spec, B, dtype=a.dtype)
    tdt = torch.float32 if a.dtype == "f32" else torch.float64
    w = 4 if a.dtype == "f32" else 8
    rng = np.random.default_rng(1)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(gm.np_dtype))).cuda()
    e = lambda *shape, dt=tdt: torch.empty(shape, dtype=dt, device="cuda")
    stream = api.torch_stream()
    L = api.lib()

    def theta(lead):
        Ws = [rng.standard_normal(lead + (widths[l], widths[l - 1])) / np.sqrt(widths[l - 1]) for l in range(1, len(widths))]
        bs = [0.1 * rng.standard_normal(lead + (widths[l],)) for l in range(1, len(widths))]
        return dev(api.pack_mlp(Ws, bs)[0])

    z0 = dev(d.synthetic_inputs(spec, B)[0])
    th_s, th_e = theta(()), theta((B,))
    W_s, W_e, b_s, b_e = (dev(0.1 * rng.standard_normal(s)) for s in ((na, nobs), (B, na, nobs), (na,), (B, na)))
    mean, scale = dev(0.1 * rng.standard_normal(nobs)), dev(rng.uniform(0.5, 1.5, nobs))

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); e1.synchronize(); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def uff(H):
        U = np.zeros((H, B, nu)); U[:, :, act_off:] = 0.2 * rng.standard_normal((H, B, na))
        return dev(U)

    res = {"tool": "mlp_policy_bench", "mechanism": spec.name, "dtype": a.dtype, "batch": B, "widths": widths, "parameters": Pn, "hidden_units": nh}

    # ---- forward ----
    H = a.steps
    Uff = uff(H)
    Z, st, OBS, U, ACT = e(H, B, nz), e(H, B, dt=torch.int32), e(H + 1, B, nobs), e(H, B, nu), e(H, B, nh, dt=torch.float64)
    mlp_s = api.mlp_policy_struct(th_s.data_ptr(), mean.data_ptr(), scale.data_ptr(), Uff.data_ptr(), 0, act_off, widths)
    mlp_e = api.mlp_policy_struct(th_e.data_ptr(), mean.data_ptr(), scale.data_ptr(), Uff.data_ptr(), 1, act_off, widths)
    aff_e = api.DojoPolicy(W_e.data_ptr(), b_e.data_ptr(), mean.data_ptr(), scale.data_ptr(), Uff.data_ptr(), 1, act_off, na, 0, 0, 0)
    closed_s = lambda: api._chk(L.dojo_rollout_mlp_dev(gm.h, api.addr(z0), C.byref(mlp_s), H, api.addr(Z), api.addr(OBS), api.addr(U), api.addr(ACT), api.addr(st), stream))
    closed_e = lambda: api._chk(L.dojo_rollout_mlp_dev(gm.h, api.addr(z0), C.byref(mlp_e), H, api.addr(Z), api.addr(OBS), api.addr(U), api.addr(ACT), api.addr(st), stream))
    affine = lambda: api._chk(L.dojo_rollout_policy_dev(gm.h, api.addr(z0), C.byref(aff_e), H, api.addr(Z), api.addr(OBS), api.addr(U), api.addr(st), stream))
    closed_s(); torch.cuda.synchronize()                        # warm-up: code objects, workspaces, the streams of the environment groups
    Urec = U.clone(); solved = int((st == 0).sum().item())
    open_loop = lambda: api._chk(L.dojo_rollout_dev(gm.h, api.addr(z0), api.addr(Urec), H, api.addr(Z), api.addr(st), stream))
    for f in (open_loop, closed_e, affine):
        f(); torch.cuda.synchronize()
    ta, tb, tc, td = [], [], [], []
    for _ in range(a.rounds):
        ta.append(timed(open_loop)); tb.append(timed(closed_s)); tc.append(timed(closed_e)); td.append(timed(affine))
        td.append(timed(affine)); tc.append(timed(closed_e)); tb.append(timed(closed_s)); same = bool(torch.equal(U, Urec)); ta.append(timed(open_loop))
    ma, mb, mc, md = (statistics.mean(t) for t in (ta, tb, tc, td))
    rate = lambda m: round(H * B / (m * 1e-3))
    res.update({"forward_steps": H, "rounds": a.rounds, "solved_env_steps": solved, "env_steps": H * B, "controls_reproduced": same,
                "open_loop_ms": round(ma, 3), "open_loop_ms_runs": [round(t, 3) for t in ta],
                "mlp_shared_ms": round(mb, 3), "mlp_shared_ms_runs": [round(t, 3) for t in tb],
                "mlp_per_env_ms": round(mc, 3), "mlp_per_env_ms_runs": [round(t, 3) for t in tc],
                "affine_per_env_ms": round(md, 3), "affine_per_env_ms_runs": [round(t, 3) for t in td],
                "open_loop_env_steps_per_s": rate(ma), "mlp_shared_env_steps_per_s": rate(mb), "mlp_per_env_env_steps_per_s": rate(mc), "affine_per_env_env_steps_per_s": rate(md),
                "ratio_mlp_shared_over_open": round(mb / ma, 4), "ratio_mlp_per_env_over_open": round(mc / ma, 4), "ratio_affine_over_open": round(md / ma, 4),
                "forward_condition_ratio_le": 1.10})
    res["forward_condition_met"] = bool(res["ratio_mlp_shared_over_open"] <= 1.10)
    runs = lambda t, k=1: " ".join("%.3f" % (x / k) for x in t)
    print("%s %s  B = %d  widths %s  P = %d  nh = %d" % (spec.name, a.dtype, B, widths, Pn, nh))
    print("forward, H = %d   %d of %d environment-steps solved (shared network)" % (H, solved, H * B))
    print("(A) open loop, recorded controls       %9.3f ms per rollout  %9.0f env-steps/s   (runs: %s)" % (ma, rate(ma), runs(ta)))
    print("(B) network, shared                    %9.3f ms per rollout  %9.0f env-steps/s   (runs: %s)" % (mb, rate(mb), runs(tb)))
    print("(C) network, one per environment       %9.3f ms per rollout  %9.0f env-steps/s   (runs: %s)" % (mc, rate(mc), runs(tc)))
    print("(D) affine, one per environment        %9.3f ms per rollout  %9.0f env-steps/s   (runs: %s)" % (md, rate(md), runs(td)))
    print("    (B) / (A)                          %9.3f                condition <= 1.10: %s" % (res["ratio_mlp_shared_over_open"], "met" if res["forward_condition_met"] else "MISSED"))
    print("    (C) / (A)  %.3f     (D) / (A)  %.3f   (other trajectories than (A)'s: for information)" % (res["ratio_mlp_per_env_over_open"], res["ratio_affine_over_open"]))
    del Z, st, OBS, U, ACT, Urec, Uff

    # ---- reverse ----
    H = a.rsteps
    Uff = uff(H)
    Z, st, OBS, U, ACT = e(H, B, nz), e(H, B, dt=torch.int32), e(H + 1, B, nobs), e(H, B, nu), e(H, B, nh, dt=torch.float64)
    DZ, DU = e(H, B, nx, nx), e(H, B, nu, nx)
    G, Gu, Go = dev(rng.standard_normal((H, B, nz))), dev(rng.standard_normal((H, B, nu))), dev(rng.standard_normal((H + 1, B, nobs)))
    gth_s, gth_e, gU, gz = e(Pn), e(B, Pn), e(H, B, nu), e(B, nx)
    gW_s, gW_e, gb_s, gb_e = e(na, nobs), e(B, na, nobs), e(na), e(B, na)
    mlp_s = api.mlp_policy_struct(th_s.data_ptr(), mean.data_ptr(), scale.data_ptr(), Uff.data_ptr(), 0, act_off, widths)
    mlp_e = api.mlp_policy_struct(th_e.data_ptr(), mean.data_ptr(), scale.data_ptr(), Uff.data_ptr(), 1, act_off, widths)
    aff_s = api.DojoPolicy(W_s.data_ptr(), b_s.data_ptr(), mean.data_ptr(), scale.data_ptr(), Uff.data_ptr(), 0, act_off, na, 0, 0, 0)
    aff_e = api.DojoPolicy(W_e.data_ptr(), b_e.data_ptr(), mean.data_ptr(), scale.data_ptr(), Uff.data_ptr(), 1, act_off, na, 0, 0, 0)
    madj = lambda g: api.DojoMlpAdjoint(DZ.data_ptr(), DU.data_ptr(), OBS.data_ptr(), ACT.data_ptr(), st.data_ptr(), z0.data_ptr(), Z.data_ptr(), None, G.data_ptr(),
                                        Gu.data_ptr(), Go.data_ptr(), g.data_ptr(), gU.data_ptr(), gz.data_ptr(), 1, 0)
    aadj = lambda gW, gb: api.DojoPolicyAdjoint(DZ.data_ptr(), DU.data_ptr(), OBS.data_ptr(), st.data_ptr(), z0.data_ptr(), Z.data_ptr(), None, G.data_ptr(), Gu.data_ptr(),
                                                Go.data_ptr(), gW.data_ptr(), gb.data_ptr(), gU.data_ptr(), gz.data_ptr(), 1, 0)
    ms, me, as_, ae = madj(gth_s), madj(gth_e), aadj(gW_s, gb_s), aadj(gW_e, gb_e)
    legs = [
        ("a", lambda: api._chk(L.dojo_rollout_mlp_record_dev(gm.h, api.addr(z0), C.byref(mlp_s), H, api.addr(Z), api.addr(OBS), api.addr(U), api.addr(ACT), api.addr(st), api.addr(DZ), api.addr(DU), stream))),
        ("b", lambda: api._chk(L.dojo_rollout_mlp_adjoint_dev(gm.h, C.byref(mlp_s), H, C.byref(ms), stream))),
        ("c", lambda: api._chk(L.dojo_rollout_mlp_adjoint_dev(gm.h, C.byref(mlp_e), H, C.byref(me), stream))),
        ("d", lambda: api._chk(L.dojo_rollout_policy_adjoint_dev(gm.h, C.byref(aff_s), H, C.byref(as_), stream))),
        ("e", lambda: api._chk(L.dojo_rollout_policy_adjoint_dev(gm.h, C.byref(aff_e), H, C.byref(ae), stream))),
    ]
    for _, f in legs:
        f()
    torch.cuda.synchronize()                                    # warm-up of each
    t = {k: [] for k, _ in legs}
    for _ in range(a.reps):
        for k, f in legs:
            t[k].append(timed(f))
    ok_steps = int((st == 0).sum().item())
    finite = bool(all(torch.isfinite(x).all().item() for x in (gth_s, gth_e, gW_s, gW_e, gb_s, gb_e, gU, gz)))
    med = {k: statistics.median(v) / H for k, v in t.items()}
    m_bytes = (H + 1) * B * nobs * 24 * 8
    rec_bytes = ok_steps * nx * (nx + nu) * w
    ws_bytes = (H - 1) * B * Pn * 16
    res.update({"reverse_steps": H, "reps": a.reps, "record_bytes": H * B * nx * (nx + nu) * w, "observation_jacobian_bytes": m_bytes, "activation_bytes": H * B * nh * 8,
                "accumulator_workspace_bytes": B * Pn * 8, "accumulator_traffic_bytes": ws_bytes, "reverse_solved_env_steps": ok_steps, "outputs_finite": finite,
                "record_ms_per_step": round(med["a"], 4), "record_ms_per_step_runs": [round(x / H, 4) for x in t["a"]],
                "mlp_shared_sweep_ms_per_step": round(med["b"], 4), "mlp_shared_sweep_ms_per_step_runs": [round(x / H, 4) for x in t["b"]],
                "mlp_per_env_sweep_ms_per_step": round(med["c"], 4), "mlp_per_env_sweep_ms_per_step_runs": [round(x / H, 4) for x in t["c"]],
                "affine_shared_sweep_ms_per_step": round(med["d"], 4), "affine_shared_sweep_ms_per_step_runs": [round(x / H, 4) for x in t["d"]],
                "affine_per_env_sweep_ms_per_step": round(med["e"], 4), "affine_per_env_sweep_ms_per_step_runs": [round(x / H, 4) for x in t["e"]],
                "mlp_shared_sweep_tb_per_s": round((rec_bytes + m_bytes + ws_bytes) / (med["b"] * H * 1e-3) / 1e12, 3),
                "ratio_mlp_shared_sweep_over_record": round(med["b"] / med["a"], 4), "ratio_mlp_per_env_sweep_over_record": round(med["c"] / med["a"], 4),
                "ratio_affine_shared_sweep_over_record": round(med["d"] / med["a"], 4), "ratio_affine_per_env_sweep_over_record": round(med["e"] / med["a"], 4),
                "reverse_condition_ratio_le": 0.25})
    res["reverse_condition_met"] = bool(res["ratio_mlp_shared_sweep_over_record"] <= 0.25)
    print("reverse, H = %d   record %.2f GB + M %.2f GB + ACT %.3f GB + accumulators %.3f GB   %d of %d environment-steps solved"
          % (H, res["record_bytes"] / 1e9, m_bytes / 1e9, res["activation_bytes"] / 1e9, res["accumulator_workspace_bytes"] / 1e9, ok_steps, H * B))
    print("(a) recording rollout, shared network          %8.3f ms per step   (runs: %s)" % (med["a"], runs(t["a"], H)))
    print("(b) network sweep + M prepass + reduction      %8.3f ms per step   (runs: %s)   %.2f TB/s of DZ + DU + M + accumulators" % (med["b"], runs(t["b"], H), res["mlp_shared_sweep_tb_per_s"]))
    print("(c) network sweep + M prepass, one per env     %8.3f ms per step   (runs: %s)" % (med["c"], runs(t["c"], H)))
    print("(d) affine sweep + M prepass + reduction       %8.3f ms per step   (runs: %s)" % (med["d"], runs(t["d"], H)))
    print("(e) affine sweep + M prepass, one per env      %8.3f ms per step   (runs: %s)" % (med["e"], runs(t["e"], H)))
    print("    (b) / (a)                                  %8.3f              condition <= 0.25: %s" % (res["ratio_mlp_shared_sweep_over_record"], "met" if res["reverse_condition_met"] else "MISSED"))
    print("    (c) / (a)  %.3f     (d) / (a)  %.3f     (e) / (a)  %.3f" % (res["ratio_mlp_per_env_sweep_over_record"], res["ratio_affine_shared_sweep_over_record"], res["ratio_affine_per_env_sweep_over_record"]))
    print(json.dumps(res))
    gm.close()
    return 0 if res["forward_condition_met"] and res["reverse_condition_met"] and same and finite else 1


if __name__ == "__main__":
    sys.exit(main())
