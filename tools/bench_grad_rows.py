"""What the gradient envelope's global rows cost (ForwardPlan grad_rows).

    python tools/bench_grad_rows.py                      # -> profiles/grad_rows/bench_grad_rows.json
    python tools/bench_grad_rows.py --parent DIR         # adds the default path of this tree against DIR's

Legs, each a child process of its own under a time limit (a leg that faults or hangs ends the run; nothing more is
started on the device after it), timed inside the child with synchronised wall time, medians of --reps repeats
after --warmup warm-ups, the two sides of a comparison alternated:

  both     headline (m = 2, n = 256, N = 1024, S = 16), value+gradient at B = 1 and B = 128: grad_rows "staged" (the
           default plan: staged rows, staged lines), "global" (global rows, streamed lines) and, for the streaming's
           own share, the forward of both plans
  stress   the stress model (m = 3, n = 1024, N = 4096, S = 32), which "staged" refuses, under "auto":
           value+gradient at B = 256 and B = 1, the same plan's forward alone, and the forward's stage times
           (dkg_plan_time_stage: cross, covariance, envelope)
  default  (--parent DIR: a checkout of the parent commit, built) the default mode of this tree against the parent's,
           --pairs alternated pairs of processes: tools/b1_probe.py's B = 1 value+gradient device chain and the
           headline B = 128 value+gradient; the spread of the parent's own medians across its processes is the
           yardstick for the difference
"""

import argparse
import ast
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 240


def _setup(root):
    sys.path[:0] = [root, os.path.join(root, "decoupled-kg_amd")]
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_rows.py needs a ROCm device: there is no CPU timing of a GPU path")
    return torch


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def alternate(torch, legs, reps, warmup):
    times = {k: [] for k in legs}
    for r in range(warmup + reps):
        for k, fn in legs.items():
            t = timed(torch, fn)
            if r >= warmup:
                times[k].append(t)
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "reps": len(v)} for k, v in times.items()}


def _headline(torch, B):
    from dkg_amd.gp_state import DeviceGPState
    from dkg_amd.synthetic import WORKLOADS, make_problem

    model, D, X, W = make_problem(WORKLOADS["headline"])
    return DeviceGPState(model, D, device="cuda:0"), W, X[:B].to("cuda:0").contiguous()


def leg_both(a):
    torch = _setup(REPO)
    res = {}
    for B in (1, 128):
        st, W, X = _headline(torch, B)
        plans = {mode: st.plan(W, None, B, grad=True, grad_rows=mode) for mode in ("staged", "global")}
        assert plans["global"].grad_rows_global and not plans["staged"].grad_rows_global
        ref = plans["staged"].forward_grad(X)
        got = plans["global"].forward_grad(X)
        legs = {f"value_grad_{m}": (lambda p=p: p.forward_grad(X)) for m, p in plans.items()}
        kg = torch.empty(B, dtype=torch.double, device="cuda:0")
        legs.update({f"forward_{m}": (lambda p=p: p.forward_into(X, kg)) for m, p in plans.items()})
        r = alternate(torch, legs, a.reps, a.warmup)
        r["envelope"] = {m: p.envelope_geometry() for m, p in plans.items()}
        r["max_abs_diff_kg"] = float((ref[0] - got[0]).abs().max())
        r["max_abs_diff_grad"] = float((ref[1] - got[1]).abs().max())
        r["ratio_global_over_staged"] = r["value_grad_global"]["median_us"] / r["value_grad_staged"]["median_us"]
        res[f"B{B}"] = r
    print(json.dumps(res))


def leg_stress(a):
    torch = _setup(REPO)
    from dkg_amd.errors import UnsupportedError
    from dkg_amd.gp_state import DeviceGPState
    from dkg_amd.synthetic import WORKLOADS, make_problem

    w = WORKLOADS["stress"]
    model, D, X, W = make_problem(w)
    st = DeviceGPState(model, D, device="cuda:0")
    try:
        st.plan(W, None, 1, grad=True)
        refused = False
    except UnsupportedError:
        refused = True
    res = {"staged_refused": refused}
    for B in (256, 1):
        Xd = X[:B].to("cuda:0").contiguous()
        plan = st.plan(W, None, B, grad=True, grad_rows="auto")
        kg = torch.empty(B, dtype=torch.double, device="cuda:0")
        r = alternate(torch, {"value_grad_auto": lambda: plan.forward_grad(Xd),
                              "forward_same_plan": lambda: plan.forward_into(Xd, kg)}, a.reps, a.warmup)
        r["grad_rows_global"] = plan.grad_rows_global
        r["envelope"] = plan.envelope_geometry()
        r["forward_stage_ms"] = {name: plan.time_stage(Xd, s, 10)
                                 for s, name in enumerate(("cross", "covariance", "envelope"))}
        res[f"B{B}"] = r
    print(json.dumps(res))


def leg_b128(a):
    """The headline B = 128 value+gradient of the tree at --root in its default mode (the parent has no other)."""
    torch = _setup(a.root)
    st, W, X = _headline(torch, 128)
    plan = st.plan(W, None, 128, grad=True)
    print(json.dumps(alternate(torch, {"value_grad": lambda: plan.forward_grad(X)}, a.reps, a.warmup)["value_grad"]))


def child(args, what):
    """One GPU step: a fresh process under its own time limit; its last output line."""
    p = subprocess.run(args, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
    if p.returncode != 0:
        raise SystemExit(f"{what}: exit status {p.returncode}; stopping (nothing more is run on the device)\n"
                         f"{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return p.stdout.strip().splitlines()[-1]


def default_path(a):
    roots = {"parent": os.path.abspath(a.parent), "new": REPO}
    b1 = {k: [] for k in roots}
    b128 = {k: [] for k in roots}
    for _ in range(a.pairs):
        for k, root in roots.items():
            out = child([sys.executable, os.path.join(root, "tools", "b1_probe.py"), "headline", "200"], f"b1_probe {k}")
            b1[k].append(ast.literal_eval(out)["device"])
            out = child([sys.executable, os.path.abspath(__file__), "--leg", "b128", "--root", root, "--reps",
                         str(a.reps), "--warmup", str(a.warmup)], f"b128 {k}")
            b128[k].append(json.loads(out)["median_us"])
            print(f"{k}: B=1 device chain {b1[k][-1]} us, B=128 value+gradient {b128[k][-1]:.1f} us", flush=True)

    def summary(v):
        s = {k: {"medians_us": x, "median_us": statistics.median(x), "spread_us": max(x) - min(x)}
             for k, x in v.items()}
        s["new_minus_parent_us"] = s["new"]["median_us"] - s["parent"]["median_us"]
        s["within_parent_spread"] = s["new_minus_parent_us"] <= s["parent"]["spread_us"]
        return s

    return {"pairs": a.pairs, "b1_device_chain": summary(b1), "b128_value_grad": summary(b128)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--parent", help="a built checkout of the parent commit: measures the default path against it")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grad_rows", "bench_grad_rows.json"))
    ap.add_argument("--leg", choices=("both", "stress", "b128"), help="(internal) run one leg in this process")
    ap.add_argument("--root", default=REPO, help="(internal, --leg b128) the tree to import")
    a = ap.parse_args()
    if a.leg:
        return {"both": leg_both, "stress": leg_stress, "b128": leg_b128}[a.leg](a)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--warmup", str(a.warmup)]
    res["timing"] = "synchronised wall time, medians, legs alternated, one process per leg"
    res["headline_staged_vs_global"] = json.loads(child(me + ["--leg", "both"], "both"))
    print(json.dumps(res["headline_staged_vs_global"], indent=1), flush=True)
    res["stress_auto"] = json.loads(child(me + ["--leg", "stress"], "stress"))
    print(json.dumps(res["stress_auto"], indent=1), flush=True)
    if a.parent:
        res["default_path_vs_parent"] = default_path(a)
        print(json.dumps(res["default_path_vs_parent"], indent=1), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
