#!/usr/bin/env python3
"""The Riccati backward pass of batched iLQR: what the one-launch kernel costs next to the calls that produce its Jacobians and next to the same recursion in torch.

Workload (default): Ant, fp32, B = 4096, H = 20, the policy drives the inputs 6 .. 13 (n = 28, na = 8).  The Jacobians are real ones: H chained calls of
dojo_minimal_gradients_dev from the synthetic start of bench.py.  Cost: lxx = I, luu = I, lx, lu ~ N(0, 1) (seeded), no regularisation.
Method: every leg is enqueued on one stream between hipEvents (torch.cuda.Event) after one warm-up of each; `--reps` repetitions, alternating the three legs in
one process; the median of each is reported with min .. max.
  (a) the H calls of dojo_minimal_gradients_dev that produce A, Bm,
  (b) the Riccati launch (dojo_riccati_dev, csrc/dojo_riccati.hpp),
  (c) the same recursion written with torch on the device in fp64 (bmm, torch.linalg.cholesky_ex, cholesky_solve) over fp64 copies of the same inputs made outside
      the timed region: what a user has without the kernel.
Checks: on a seeded well-conditioned problem of the same shape (A = I + 0.1 N / sqrt(n), B = N / sqrt(n), lxx = M M' + 0.1 I, luu = M M' + I, eight environments)
(c) must agree with a NumPy recursion to 1e-9 and the kernel with (c) to 1e-9 (fp64 handles) or 1e-5 (fp32: its inputs and outputs are rounded).  On the timed
problem itself the agreement of (b) and (c) is reported, not gated: its Jacobians are real ones (contacts in force), whose conditioning nobody controls.
Condition (the tool exits with status 1 when it is missed): (b) < (c) by more than the spread (max - min) of (c).  (b) / (a) is reported, not gated.
A second workload (default: Atlas, n = 72, na = 30 at offset 6, B = 2048) is reported only.  With --out the lines are written to that file as well.
Needs a GPU: there is no fallback.

    python tools/riccati_bench.py [--batch 4096] [--steps 20] [--dtype f32] [--reps 7] [--config 3] [--second-config 5 --second-batch 2048] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dojo.jl_amd", "host"))


def numpy_recursion(A, Bm, lx, lu, lxx, luu):
    """the recursion for one environment, fp64 NumPy (failed steps: zero Jacobians are passed in) -> K [H,m,n], kff [H,m], dV [2]"""
    import numpy as np
    H = A.shape[0]
    Vx, Vxx, dV = lx[H], lxx[H], np.zeros(2)
    K, kff = np.zeros((H,) + (Bm.shape[2], A.shape[1])), np.zeros((H, Bm.shape[2]))
    for k in range(H - 1, -1, -1):
        Qx, Qu = lx[k] + A[k].T @ Vx, lu[k] + Bm[k].T @ Vx
        Qxx, Qux, Quu = lxx[k] + A[k].T @ Vxx @ A[k], Bm[k].T @ Vxx @ A[k], luu[k] + Bm[k].T @ Vxx @ Bm[k]
        kff[k] = -np.linalg.solve(Quu, Qu); K[k] = -np.linalg.solve(Quu, Qux)
        dV += [kff[k] @ Qu, 0.5 * kff[k] @ Quu @ kff[k]]
        Vx = Qx + K[k].T @ Quu @ kff[k] + K[k].T @ Qu + Qux.T @ kff[k]
        Vxx = Qxx + K[k].T @ Quu @ K[k] + K[k].T @ Qux + Qux.T @ K[k]
        Vxx = 0.5 * (Vxx + Vxx.T)
    return K, kff, dV


def torch_recursion(torch, A, Bm, lx, lu, lxx, luu):
    """leg (c): fp64 device tensors A [H,B,n,n], Bm [H,B,n,m] (zeros at failed steps) -> K [H,B,m,n], kff [H,B,m], dV [B,2], info [H,B]"""
    H, B = A.shape[:2]
    Vx, Vxx = lx[H], lxx[H]
    dV = torch.zeros((B, 2), dtype=A.dtype, device=A.device)
    Ks, ks, infos = [None] * H, [None] * H, [None] * H
    for k in range(H - 1, -1, -1):
        At, Bt = A[k].transpose(1, 2), Bm[k].transpose(1, 2)
        Qx = lx[k] + torch.bmm(At, Vx[..., None])[..., 0]; Qu = lu[k] + torch.bmm(Bt, Vx[..., None])[..., 0]
        AtV, BtV = torch.bmm(At, Vxx), torch.bmm(Bt, Vxx)
        Qxx = lxx[k] + torch.bmm(AtV, A[k]); Qux = torch.bmm(BtV, A[k]); Quu = luu[k] + torch.bmm(BtV, Bm[k])
        L, infos[k] = torch.linalg.cholesky_ex(Quu)
        sol = -torch.cholesky_solve(torch.cat([Qu[..., None], Qux], -1), L)
        kff, K = sol[..., 0], sol[..., 1:]
        Kt = K.transpose(1, 2)
        Quu_k = torch.bmm(Quu, kff[..., None])[..., 0]
        dV[:, 0] += (kff * Qu).sum(-1); dV[:, 1] += 0.5 * (kff * Quu_k).sum(-1)
        Vx = Qx + torch.bmm(Kt, (Quu_k + Qu)[..., None])[..., 0] + torch.bmm(Qux.transpose(1, 2), kff[..., None])[..., 0]
        KtQux = torch.bmm(Kt, Qux)
        Vxx = Qxx + torch.bmm(Kt, torch.bmm(Quu, K)) + KtQux + KtQux.transpose(1, 2)
        Vxx = 0.5 * (Vxx + Vxx.transpose(1, 2))
        Ks[k], ks[k] = K, kff
    return torch.stack(Ks), torch.stack(ks), dV, torch.stack(infos)


def validate(torch, np, d, api, spec, a, act_off, na):
    """(c) against NumPy and the kernel against (c) on a seeded well-conditioned problem of the timed shape -> (rel. error of (c), rel. difference of the kernel)"""
    Bv, H, nu = 8, a.steps, spec.nu
    n = 2 * nu
    rng = np.random.default_rng(7)
    A = np.eye(n) + 0.1 * rng.standard_normal((H, Bv, n, n)) / np.sqrt(n); Bm = rng.standard_normal((H, Bv, n, nu)) / np.sqrt(n)
    M = rng.standard_normal((H + 1, Bv, n, n)); lxx = M @ M.transpose(0, 1, 3, 2) + 0.1 * np.eye(n)
    M = rng.standard_normal((H, Bv, na, na)); luu = M @ M.transpose(0, 1, 3, 2) + np.eye(na)
    lx, lu = rng.standard_normal((H + 1, Bv, n)), rng.standard_normal((H, Bv, na))
    gm = api.BatchedMechanism(spec, Bv, dtype=a.dtype)
    arrs = [np.ascontiguousarray(x.astype(gm.np_dtype)) for x in (A, Bm, lx, lu, lxx, luu)]
    K, kff, dV, fail = gm.riccati(*arrs, act_off=act_off, na=na, value=False)
    gm.close()
    c_in = [torch.from_numpy(x.astype(np.float64)).cuda() for x in arrs]
    c_in[1] = c_in[1][..., act_off:act_off + na].contiguous()
    Kc, kc, dVc, info = torch_recursion(torch, *c_in)
    e_np = 0.0
    for b in range(Bv):
        Kn, kn, dVn = numpy_recursion(*[t[:, b].cpu().numpy() for t in c_in])
        e_np = max(e_np, float(np.abs(Kn - Kc[:, b].cpu().numpy()).max() / np.abs(Kn).max()), float(np.abs(dVn - dVc[b].cpu().numpy()).max() / np.abs(dVn).max()))
    e_k = max(float(np.abs(K - Kc.cpu().numpy()).max() / np.abs(K).max()), float(np.abs(dV - dVc.cpu().numpy()).max() / np.abs(dV).max()))
    return e_np, e_k, int(fail.any()) + int(info.any().item())


def measure(a, config, B, act_off, na, gated):
    import numpy as np
    import torch
    import dojo_amd as d
    from dojo_amd import api

    spec = d.baseline_config(config)
    H, nu = a.steps, spec.nu
    n = 2 * nu
    na = nu - act_off if na is None else na
    e_np, e_k, v_fail = validate(torch, np, d, api, spec, a, act_off, na)
    gm = api.BatchedMechanism(spec, B, dtype=a.dtype)
    tdt = torch.float32 if a.dtype == "f32" else torch.float64
    z0, u = d.synthetic_inputs(spec, B)
    rng = np.random.default_rng(1)
    U = np.stack([u * rng.uniform(0.5, 1.0) for _ in range(H)])
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(gm.np_dtype))).cuda()
    empty = lambda *shape: torch.empty(shape, dtype=tdt, device="cuda")
    X = empty(H + 1, B, n); X[0] = dev(gm.maximal_to_minimal(z0.astype(gm.np_dtype)))
    Ud = dev(U)
    A, Bm = empty(H, B, n, n), empty(H, B, n, nu)
    st = torch.empty((H, B), dtype=torch.int32, device="cuda"); it = torch.empty(B, dtype=torch.int32, device="cuda")
    lx, lu = dev(rng.standard_normal((H + 1, B, n))), dev(rng.standard_normal((H, B, na)))
    lxx = torch.eye(n, dtype=tdt, device="cuda").expand(H + 1, B, n, n).contiguous(); luu = torch.eye(na, dtype=tdt, device="cuda").expand(H, B, na, na).contiguous()
    K, kff, dV, fail = empty(H, B, na, n), empty(H, B, na), empty(B, 2), torch.empty(B, dtype=torch.int32, device="cuda")
    stream = api.torch_stream()
    L = api.lib()
    rec = api.DojoRiccati(A.data_ptr(), Bm.data_ptr(), st.data_ptr(), lx.data_ptr(), lu.data_ptr(), lxx.data_ptr(), luu.data_ptr(), None, None,
                          K.data_ptr(), kff.data_ptr(), fail.data_ptr(), dV.data_ptr(), None, None, act_off, na)

    def linearize():
        for k in range(H):
            api._chk(L.dojo_minimal_gradients_dev(gm.h, api.addr(X[k]), api.addr(Ud[k]), api.addr(X[k + 1]), api.addr(st[k]), api.addr(it), api.addr(A[k]), api.addr(Bm[k]), stream))

    def kernel():
        api._chk(L.dojo_riccati_dev(gm.h, H, C.byref(rec), stream))

    linearize()                                                             # (warm-up of (a), and the inputs of (b), (c))
    torch.cuda.synchronize()
    ok = (st == 0)
    A64 = torch.where(ok[..., None, None], A.double(), torch.zeros((), dtype=torch.float64, device="cuda"))
    B64 = torch.where(ok[..., None, None], Bm[..., act_off:act_off + na].double(), torch.zeros((), dtype=torch.float64, device="cuda")).contiguous()
    c_in = (A64, B64, lx.double(), lu.double(), lxx.double(), luu.double())
    c_out = [None]

    def torch_leg():
        c_out[0] = torch_recursion(torch, *c_in)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    calls = [("a", linearize), ("b", kernel), ("c", torch_leg)]
    kernel(); torch_leg()                                                   # warm-up of (b) and (c)
    torch.cuda.synchronize()
    runs = {k: [] for k, _ in calls}
    for _ in range(a.reps):
        for k, f in calls:
            runs[k].append(timed(f))
    # (b) against (c) on the timed problem, over the environments neither of them gave up on: reported only
    Kc, kc, dVc, info = c_out[0]
    good = (fail == 0) & (info == 0).all(0)
    scale = Kc[:, good].abs().amax(dim=(0, 2, 3)).clamp_min(1e-300)
    per_env = (K.double() - Kc)[:, good].abs().amax(dim=(0, 2, 3)) / scale
    diff_bc, diff_bc_med = (float(per_env.max().item()), float(per_env.median().item())) if bool(good.any()) else (float("nan"), float("nan"))
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread_c = max(runs["c"]) - min(runs["c"])
    res = {"tool": "riccati_bench", "mechanism": spec.name, "dtype": a.dtype, "batch": B, "steps": H, "n": n, "na": na, "act_off": act_off, "reps": a.reps,
           "solved_env_steps": int(ok.sum().item()), "env_steps": H * B, "kernel_failed_envs": int((fail != 0).sum().item()), "torch_failed_envs": int((info != 0).any(0).sum().item()),
           "ms": {k: round(v, 4) for k, v in med.items()}, "ms_runs": {k: [round(t, 4) for t in v] for k, v in runs.items()},
           "spread_c_ms": round(spread_c, 4), "ratio_b_over_a": round(med["b"] / med["a"], 5), "ratio_c_over_b": round(med["c"] / med["b"], 3),
           "check_torch_vs_numpy_rel": e_np, "check_kernel_vs_torch_rel": e_k, "check_failures": v_fail,
           "timed_kernel_vs_torch_rel_K_max": diff_bc, "timed_kernel_vs_torch_rel_K_median": diff_bc_med, "gated": gated}
    res["checks_passed"] = bool(e_np <= 1e-9 and e_k <= (1e-5 if a.dtype == "f32" else 1e-9) and v_fail == 0)
    res["condition_b_lt_c"] = bool(med["c"] - med["b"] > spread_c)
    names = {"a": "H x dojo_minimal_gradients_dev", "b": "dojo_riccati_dev, one launch  ", "c": "torch fp64 recursion         "}
    lines = ["%s %s  B = %d  H = %d  n = %d  na = %d (inputs %d .. %d)   %d of %d environment-steps solved; Cholesky failures: kernel %d, torch %d environments"
             % (spec.name, a.dtype, B, H, n, na, act_off, act_off + na - 1, res["solved_env_steps"], H * B, res["kernel_failed_envs"], res["torch_failed_envs"])]
    for k, _ in calls:
        lines.append("(%s) %s %9.3f ms   (min %.3f .. max %.3f; runs: %s)" % (k, names[k], med[k], min(runs[k]), max(runs[k]), " ".join("%.3f" % t for t in runs[k])))
    lines.append("(c) / (b) = %.1f   (b) < (c) by more than the spread of (c) (%.3f ms): %s%s" % (res["ratio_c_over_b"], spread_c, "met" if res["condition_b_lt_c"] else "MISSED", "" if gated else "   (reported only)"))
    lines.append("(b) / (a) = %.4f   (reported, not gated)" % res["ratio_b_over_a"])
    lines.append("checks on the seeded well-conditioned problem of this shape: (c) against NumPy %.1e, kernel against (c) %.1e (relative): %s" % (e_np, e_k, "passed" if res["checks_passed"] else "FAILED"))
    lines.append("on the timed problem, K of (b) against (c) relative to each environment's largest gain: median %.1e, max %.1e   (reported only)" % (diff_bc_med, diff_bc))
    lines.append(json.dumps(res))
    gm.close()
    del c_in, c_out, A64, B64
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
        raise SystemExit("riccati_bench: no GPU")
    torch.cuda.init()
    res, lines = measure(a, a.config, a.batch, a.act_off, a.na, True)
    if a.second_config:
        _, more = measure(a, a.second_config, a.second_batch, 6, None, False)
        lines += [""] + more
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if res["condition_b_lt_c"] and res["checks_passed"] else 1


if __name__ == "__main__":
    sys.exit(main())
