#!/usr/bin/env python3
"""The control-limited Riccati backward pass (dojo_riccati_box_dev, include/dojo_hip_limits.h) next to the unconstrained one it extends.

Workload (default): the shape of Ant, fp32, B = 4096, H = 20, the inputs 6 .. 13 driven (n = 28, na = 8), and a second one, reported alike: Atlas, B = 2048
(n = 72, na = 30).  Inputs: the seeded family of the tests (tests/riccati_cases.py: A = I + 0.1 N / sqrt(n), B = N / sqrt(n), lxx = M M' + 0.1 I, luu = M M' + I,
lux = 0.1 N, lx, lu ~ N; tests/box_cases.py: U = clip(0.5 N, -c, c)), the same arrays for all three legs.  Nothing is stepped: the handle only gives the shape.
Method: every leg is one launch enqueued on one stream between hipEvents (torch.cuda.Event) after one warm-up of each; `--reps` repetitions, alternating the
three legs in one process; the median of each is reported with min .. max.
  (a) dojo_riccati_dev,
  (b) dojo_riccati_box_dev with lo = -inf, hi = +inf: no step's start point is clipped, so its extra work over (a) is the clip test of every step,
  (c) dojo_riccati_box_dev with lo = -c, hi = +c, c = 0.25: the main family of the tests, where a third of the inputs end clamped.
Checks (the tool exits with status 1 when one is missed): (b) returns the bits of (a) with active = qp_iters = 0; (c) fails in no environment and clamps something.
Reported: the three times, (b) / (a), (c) / (a), the mean and the largest qp_iters of (c) and its clamped share.  No ratio is gated.
With --out the lines are written to that file as well.  Needs a GPU: there is no fallback.

    python tools/riccati_box_bench.py [--batch 4096] [--steps 20] [--dtype f32] [--reps 7] [--second-batch 2048] [--c 0.25] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dojo.jl_amd", "host"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(a, shape, config, B):
    import numpy as np
    import torch
    import dojo_amd as d
    from dojo_amd import api
    import box_cases as BC
    import riccati_cases as RC

    name, n, nu, act_off, m = RC.SHAPES[shape]
    H = a.steps
    spec = d.baseline_config(config)
    assert spec.nu == nu
    gm = api.BatchedMechanism(spec, B, dtype=a.dtype)
    tdt = torch.float32 if a.dtype == "f32" else torch.float64
    f32 = a.dtype == "f32"
    inp = RC.inputs(shape, H, B, f32)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(gm.np_dtype))).cuda()
    din = {k: dev(v) for k, v in inp.items()}
    U = dev(BC.controls(shape, H, B, a.c, f32))
    inf = torch.full((B, m), float("inf"), dtype=tdt, device="cuda")
    lims = {"b": (-inf, inf), "c": (torch.full((B, m), -a.c, dtype=tdt, device="cuda"), torch.full((B, m), a.c, dtype=tdt, device="cuda"))}

    def outputs():
        o = {"K": torch.empty((H, B, m, n), dtype=tdt, device="cuda"), "kff": torch.empty((H, B, m), dtype=tdt, device="cuda"), "fail": torch.empty(B, dtype=torch.int32, device="cuda"),
             "dV": torch.empty((B, 2), dtype=tdt, device="cuda"), "active": torch.empty((H, B), dtype=torch.int64, device="cuda"), "iters": torch.empty((H, B), dtype=torch.int32, device="cuda")}
        rec = api.DojoRiccati(*[api.addr(din[k]) for k in ("A", "Bm")], None, *[api.addr(din[k]) for k in ("lx", "lu", "lxx", "luu", "lux")], None,
                              api.addr(o["K"]), api.addr(o["kff"]), api.addr(o["fail"]), api.addr(o["dV"]), None, None, act_off, m)
        return o, rec

    outs = {k: outputs() for k in ("a", "b", "c")}
    L, stream = api.lib(), api.torch_stream()

    def leg(k):
        o, rec = outs[k]
        if k == "a":
            return lambda: api._chk(L.dojo_riccati_dev(gm.h, H, C.byref(rec), stream))
        lim = api.DojoControlLimits(api.addr(lims[k][0]), api.addr(lims[k][1]))
        return lambda: api._chk(L.dojo_riccati_box_dev(gm.h, H, C.byref(rec), C.byref(lim), api.addr(U), api.addr(o["active"]), api.addr(o["iters"]), stream))

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    calls = [(k, leg(k)) for k in ("a", "b", "c")]
    for _, f in calls:
        f()                                                                 # warm-up
    torch.cuda.synchronize()
    runs = {k: [] for k, _ in calls}
    for _ in range(a.reps):
        for k, f in calls:
            runs[k].append(timed(f))
    oa, ob, oc = outs["a"][0], outs["b"][0], outs["c"][0]
    same = all(torch.equal(oa[k].view(torch.uint8), ob[k].view(torch.uint8)) for k in ("K", "kff", "fail", "dV")) and not bool(ob["active"].any()) and not bool(ob["iters"].any())
    bitcount = sum(((oc["active"] >> i) & 1).sum() for i in range(m))
    share = float(bitcount.item()) / (H * B * m)
    med = {k: statistics.median(v) for k, v in runs.items()}
    res = {"tool": "riccati_box_bench", "mechanism": spec.name, "dtype": a.dtype, "batch": B, "steps": H, "n": n, "na": m, "act_off": act_off, "reps": a.reps, "c": a.c,
           "ms": {k: round(v, 4) for k, v in med.items()}, "ms_runs": {k: [round(t, 4) for t in v] for k, v in runs.items()},
           "ratio_b_over_a": round(med["b"] / med["a"], 4), "ratio_c_over_a": round(med["c"] / med["a"], 4),
           "qp_iters_mean_c": round(float(oc["iters"].double().mean().item()), 4), "qp_iters_max_c": int(oc["iters"].max().item()), "clamped_share_c": round(share, 4),
           "failed_envs": {k: int((outs[k][0]["fail"] != 0).sum().item()) for k in outs}, "b_has_the_bits_of_a": bool(same)}
    res["checks_passed"] = bool(same and res["failed_envs"]["c"] == 0 and share > 0)
    names = {"a": "dojo_riccati_dev                       ", "b": "dojo_riccati_box_dev, limits -inf .. inf", "c": "dojo_riccati_box_dev, limits -c .. c    "}
    lines = ["%s %s  B = %d  H = %d  n = %d  na = %d (inputs %d .. %d)   the seeded family of tests/box_cases.py, c = %g; failed environments: %s"
             % (spec.name, a.dtype, B, H, n, m, act_off, act_off + m - 1, a.c, res["failed_envs"])]
    for k, _ in calls:
        lines.append("(%s) %s %9.3f ms   (min %.3f .. max %.3f; runs: %s)" % (k, names[k], med[k], min(runs[k]), max(runs[k]), " ".join("%.3f" % t for t in runs[k])))
    lines.append("(b) / (a) = %.3f   (c) / (a) = %.3f   (reported, not gated)" % (res["ratio_b_over_a"], res["ratio_c_over_a"]))
    lines.append("(c): qp_iters mean %.3f, max %d per environment-step; %.1f %% of the inputs clamped" % (res["qp_iters_mean_c"], res["qp_iters_max_c"], 100.0 * share))
    lines.append("checks: (b) has the bits of (a), active = qp_iters = 0: %s; (c) fails nowhere and clamps: %s" % ("passed" if same else "FAILED", "passed" if res["failed_envs"]["c"] == 0 and share > 0 else "FAILED"))
    lines.append(json.dumps(res))
    gm.close()
    del din, outs
    torch.cuda.empty_cache()
    return res, lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--c", type=float, default=0.25)
    ap.add_argument("--second-batch", type=int, default=2048, help="Atlas, reported alike (0 = none)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()

    import torch                      # (first: torch brings the GPU up, INTEGRATION.md "Using the library next to PyTorch")
    if not torch.cuda.is_available():
        raise SystemExit("riccati_box_bench: no GPU")
    torch.cuda.init()
    res, lines = measure(a, "ant", 3, a.batch)
    ok = res["checks_passed"]
    if a.second_batch:
        res2, more = measure(a, "atlas", 5, a.second_batch)
        lines += [""] + more
        ok = ok and res2["checks_passed"]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
