#!/usr/bin/env python3
"""The constrained Riccati backward pass (dojo_riccati_al_dev, include/dojo_hip_constraints.h) next to the control-limited one it extends and next to forming the
augmented-Lagrangian terms in torch.

Workload (default): the shape of Ant, fp32, B = 4096, H = 20, the inputs 6 .. 13 driven (n = 28, na = 8), and a second one, reported alike: Atlas, B = 2048
(n = 72, na = 30).  Inputs: the seeded family of the tests (tests/riccati_cases.py); constraint rows nc = n: Cx, Cu = N / sqrt(n + na), w = 10^U(-1, 2), y ~ N
(torch, seeded), every row live.  Nothing is stepped: the handle only gives the shape.
Method: every leg is enqueued on one stream between hipEvents (torch.cuda.Event) after one warm-up of each; `--reps` repetitions, alternating the legs in one
process; the median of each is reported with min .. max.
  (a) dojo_riccati_box_dev with lo = -inf, hi = +inf: the code of the parent commit, the reference leg,
  (b) dojo_riccati_al_dev with nc = 0,
  (c) dojo_riccati_al_dev with a terminal goal: nc = n, shared Cx = I, live at stage H only,
  (d) dojo_riccati_al_dev with path constraints: nc = n live at every stage, per-environment Jacobians,
  (e) the terms of (d) formed into lx .. lux by torch (baddbmm_ in place on the cost arrays), then leg (a).  The cost arrays are restored outside the timing.
Conditions, judged against the spread of the reference leg, not against a fixed ratio (the tool exits with status 1 when one is missed or a check fails):
  (b) and (c) are no slower than (a) by more than (a)'s min .. max spread;  (d) is faster than (e) by more than (e)'s spread.
Checks: (b) has the bits of (a); (d) and (e) agree to the precision of the handle dtype; no leg fails in any environment.
With --out the lines are written to that file as well.  Needs a GPU: there is no fallback.

    python tools/riccati_al_bench.py [--batch 4096] [--steps 20] [--dtype f32] [--reps 7] [--second-batch 2048] [--out FILE]
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
    import riccati_cases as RC

    name, n, nu, act_off, m = RC.SHAPES[shape]
    H, nc = a.steps, n
    spec = d.baseline_config(config)
    assert spec.nu == nu
    gm = api.BatchedMechanism(spec, B, dtype=a.dtype)
    tdt = torch.float32 if a.dtype == "f32" else torch.float64
    f32 = a.dtype == "f32"
    inp = RC.inputs(shape, H, B, f32)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(gm.np_dtype))).cuda()
    din = {k: dev(v) for k, v in inp.items()}
    U = torch.zeros((H, B, nu), dtype=tdt, device="cuda")
    inf = torch.full((B, m), float("inf"), dtype=tdt, device="cuda")
    g = torch.Generator(device="cuda"); g.manual_seed(23)
    rnd = lambda *s: torch.randn(*s, dtype=tdt, device="cuda", generator=g)
    Cx, Cu = rnd(H + 1, B, nc, n) / (n + m) ** 0.5, rnd(H, B, nc, m) / (n + m) ** 0.5
    w = 10.0 ** (3.0 * torch.rand(H + 1, B, nc, dtype=tdt, device="cuda", generator=g) - 1.0); y = rnd(H + 1, B, nc)
    eye = torch.eye(n, dtype=tdt, device="cuda")
    w_term, y_term = torch.zeros_like(w), torch.zeros_like(y); w_term[H] = w[H]; y_term[H] = y[H]
    cons = {"b": api.DojoStageConstraints(None, None, None, None, 0, 0),
            "c": api.DojoStageConstraints(api.addr(eye), None, api.addr(w_term), api.addr(y_term), nc, 1),
            "d": api.DojoStageConstraints(api.addr(Cx), api.addr(Cu), api.addr(w), api.addr(y), nc, 0)}
    cost = ("lx", "lu", "lxx", "luu", "lux")
    work = {k: din[k].clone() for k in cost}                                    # leg (e) adds into these

    def outputs(src):
        o = {"K": torch.empty((H, B, m, n), dtype=tdt, device="cuda"), "kff": torch.empty((H, B, m), dtype=tdt, device="cuda"), "fail": torch.empty(B, dtype=torch.int32, device="cuda"),
             "dV": torch.empty((B, 2), dtype=tdt, device="cuda"), "active": torch.empty((H, B), dtype=torch.int64, device="cuda"), "iters": torch.empty((H, B), dtype=torch.int32, device="cuda")}
        rec = api.DojoRiccati(*[api.addr(din[k]) for k in ("A", "Bm")], None, *[api.addr(src[k]) for k in cost], None,
                              api.addr(o["K"]), api.addr(o["kff"]), api.addr(o["fail"]), api.addr(o["dV"]), None, None, act_off, m)
        return o, rec

    outs = {k: outputs(work if k == "e" else din) for k in "abcde"}
    L, stream = api.lib(), api.torch_stream()
    keep = (-inf, inf)
    lim = api.DojoControlLimits(api.addr(keep[0]), api.addr(keep[1]))

    def box(k):
        o, rec = outs[k]
        api._chk(L.dojo_riccati_box_dev(gm.h, H, C.byref(rec), C.byref(lim), api.addr(U), api.addr(o["active"]), api.addr(o["iters"]), stream))

    def al(k):
        o, rec = outs[k]
        api._chk(L.dojo_riccati_al_dev(gm.h, H, C.byref(rec), C.byref(lim), api.addr(U), C.byref(cons[k]), api.addr(o["active"]), api.addr(o["iters"]), stream))

    def torch_terms():
        HB = H * B
        wCx = w[..., None] * Cx; wCu = w[:H, ..., None] * Cu
        work["lxx"].view(-1, n, n).baddbmm_(Cx.view(-1, nc, n).transpose(1, 2), wCx.view(-1, nc, n))
        work["lux"].view(-1, m, n).baddbmm_(Cu.view(-1, nc, m).transpose(1, 2), wCx[:H].reshape(HB, nc, n))
        work["luu"].view(-1, m, m).baddbmm_(Cu.view(-1, nc, m).transpose(1, 2), wCu.view(-1, nc, m))
        work["lx"].view(-1, n, 1).baddbmm_(Cx.view(-1, nc, n).transpose(1, 2), y.view(-1, nc, 1))
        work["lu"].view(-1, m, 1).baddbmm_(Cu.view(-1, nc, m).transpose(1, 2), y[:H].reshape(HB, nc, 1))
        box("e")

    def restore():
        for k in cost:
            work[k].copy_(din[k])

    legs = {"a": lambda: box("a"), "b": lambda: al("b"), "c": lambda: al("c"), "d": lambda: al("d"), "e": torch_terms}

    def timed(k):
        if k == "e":
            restore()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); legs[k](); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    for k in legs:
        timed(k)                                                            # warm-up
    torch.cuda.synchronize()
    runs = {k: [] for k in legs}
    for _ in range(a.reps):
        for k in legs:
            runs[k].append(timed(k))
    o = {k: v[0] for k, v in outs.items()}
    same = all(torch.equal(o["a"][k].view(torch.uint8), o["b"][k].view(torch.uint8)) for k in ("K", "kff", "fail", "dV", "active", "iters"))
    rel = float(((o["d"]["K"].double() - o["e"]["K"].double()).abs().max() / o["e"]["K"].double().abs().max()).item())
    tol = 1e-2 if f32 else 1e-9                                               # (e) rounds the terms to the handle dtype in memory, (d) keeps them in fp64
    failed = {k: int((o[k]["fail"] != 0).sum().item()) for k in o}
    differs = not torch.equal(o["c"]["K"], o["a"]["K"]) and not torch.equal(o["d"]["K"], o["c"]["K"])
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = {k: max(v) - min(v) for k, v in runs.items()}
    meets = {"b": med["b"] <= med["a"] + spread["a"], "c": med["c"] <= med["a"] + spread["a"], "d": med["d"] < med["e"] - spread["e"]}
    checks = bool(same and rel <= tol and not any(failed.values()) and differs)
    res = {"tool": "riccati_al_bench", "mechanism": spec.name, "dtype": a.dtype, "batch": B, "steps": H, "n": n, "na": m, "nc": nc, "act_off": act_off, "reps": a.reps,
           "ms": {k: round(v, 4) for k, v in med.items()}, "ms_runs": {k: [round(t, 4) for t in v] for k, v in runs.items()}, "spread_ms": {k: round(v, 4) for k, v in spread.items()},
           "meets": meets, "failed_envs": failed, "b_has_the_bits_of_a": bool(same), "d_vs_e_rel_K": rel, "checks_passed": checks}
    names = {"a": "dojo_riccati_box_dev, limits -inf .. inf    ", "b": "dojo_riccati_al_dev, nc = 0                 ", "c": "dojo_riccati_al_dev, terminal goal, shared  ",
             "d": "dojo_riccati_al_dev, path rows, per env     ", "e": "torch forms the terms of (d), then leg (a)  "}
    lines = ["%s %s  B = %d  H = %d  n = %d  na = %d (inputs %d .. %d)  nc = %d   failed environments: %s" % (spec.name, a.dtype, B, H, n, m, act_off, act_off + m - 1, nc, failed)]
    for k in legs:
        lines.append("(%s) %s %9.3f ms   (min %.3f .. max %.3f; runs: %s)" % (k, names[k], med[k], min(runs[k]), max(runs[k]), " ".join("%.3f" % t for t in runs[k])))
    lines.append("(b) <= (a) + spread(a) = %.3f: %s   (c) likewise: %s   (d) < (e) - spread(e) = %.3f: %s" % (
        med["a"] + spread["a"], "MEETS" if meets["b"] else "MISSES", "MEETS" if meets["c"] else "MISSES", med["e"] - spread["e"], "MEETS" if meets["d"] else "MISSES"))
    lines.append("checks: (b) has the bits of (a): %s; |K(d) - K(e)| / max|K| = %.2e (<= %.0e): %s; no failed environment, the rows matter: %s" % (
        "passed" if same else "FAILED", rel, tol, "passed" if rel <= tol else "FAILED", "passed" if not any(failed.values()) and differs else "FAILED"))
    lines.append(json.dumps(res))
    gm.close()
    del din, outs, work, Cx, Cu, w, y
    torch.cuda.empty_cache()
    return res, lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--second-batch", type=int, default=2048, help="Atlas, reported alike (0 = none)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()

    import torch                      # (first: torch brings the GPU up, INTEGRATION.md "Using the library next to PyTorch")
    if not torch.cuda.is_available():
        raise SystemExit("riccati_al_bench: no GPU")
    torch.cuda.init()
    res, lines = measure(a, "ant", 3, a.batch)
    ok = res["checks_passed"] and all(res["meets"].values())
    if a.second_batch:
        res2, more = measure(a, "atlas", 5, a.second_batch)
        lines += [""] + more
        ok = ok and res2["checks_passed"] and all(res2["meets"].values())
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
