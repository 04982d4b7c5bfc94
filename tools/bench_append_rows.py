"""A block of observations appended to the device GP state in one batched update.

Legs, timed in one process, alternating, synchronised wall time, median of --reps repeats after --warmup
warm-ups:
  block   : state.with_observations(i, X[K], y)         -- dkg_append_rows, K = 10 rows
  chain   : ten state.with_observation(i, x, y) calls   -- dkg_append_observation
  rebuild : DeviceGPState(model of n + 10)
at the headline shape (m = 2, 246 -> 256, N = 1024) and the stress shape (m = 3, 1014 -> 1024, N = 4096), each
for a decoupled update (output 0 grows) and a full one (every output grows); and the construction of the joint
entropy search acquisition at the reference preset (P = 10 samples x 10 points, m = 2) at n = 64 and n = 256:
  append      : conditioning="append"      -- state 0's preparation, then one dkg_append_rows over P m jobs
  refactorise : conditioning="refactorise" -- P + 1 full preparations

    python tools/bench_append_rows.py                  # timings -> profiles/append_rows/bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_append_rows.py --trace
    python tools/bench_append_rows.py --kernel-stats DIR/.../run_kernel_stats.csv    # adds the per-kernel times
"""

import argparse
import csv
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "decoupled-kg_amd")]
import torch  # noqa: E402

from dkg_amd.gp_state import DeviceGPState  # noqa: E402
from dkg_amd.model import ModelListGPState, SingleTaskGPState  # noqa: E402
from dkg_amd.synthetic import WORKLOADS, make_problem  # noqa: E402

K = 10
SHAPES = ("headline", "stress")
JES_SHAPES = {"n64": "small", "n256": "headline"}  # m = 2 both
KERNELS = ("rows_copy_kernel", "rows_kx_kernel", "rows_b_kernel", "rows_w_kernel", "rows_chol_kernel",
           "rows_finish_kernel", "rows_pack_kernel", "rows_disc_kernel", "append_solve_kernel")


def head(st, n):
    return SingleTaskGPState(st.train_x[:n], st.train_y[:n], st.lengthscale, st.outputscale, st.noise,
                             st.mean_constant, st.kernel, st.nu, st.y_mean, st.y_std)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def block(state, model, outputs):
    for i in outputs:
        m = model.models[i]
        state = state.with_observations(i, m.train_x[-K:], y=m.train_y[-K:])
    return state


def chain(state, model, outputs):
    for i in outputs:
        m = model.models[i]
        for r in range(m.num_train - K, m.num_train):
            state = state.with_observation(i, m.train_x[r], y=m.train_y[r])
    return state


def cases(name):
    model, D, _, _ = make_problem(WORKLOADS[name])
    n1 = model.models[0].num_train
    dec = ModelListGPState(*[head(m, n1 - K) if i == 0 else m for i, m in enumerate(model.models)])
    full = ModelListGPState(*[head(m, n1 - K) for m in model.models])
    return model, D, {"decoupled": (dec, [0]), "full": (full, list(range(model.num_outputs)))}


def measure(name, reps, warmup):
    model, D, upd = cases(name)
    dev = torch.device("cuda", 0)
    Dd = D.to(dev)
    res = {"m": model.num_outputs, "n": model.models[0].num_train - K, "K": K, "N": D.shape[0]}
    for kind, (base_model, outputs) in upd.items():
        base = DeviceGPState(base_model, Dd, dev)
        t = {"rebuild": [], "chain": [], "block": []}
        for r in range(warmup + reps):
            tr, cold = timed(lambda: DeviceGPState(model, Dd, dev))
            tc, _ = timed(lambda: chain(base, model, outputs))
            tb, warm = timed(lambda: block(base, model, outputs))
            if r >= warmup:
                t["rebuild"].append(tr)
                t["chain"].append(tc)
                t["block"].append(tb)
        gap = max(float((a.disc_mean - b.disc_mean).abs().max() / b.disc_mean.abs().max())
                  for a, b in zip(warm.outputs, cold.outputs))
        med = {k: statistics.median(v) for k, v in t.items()}
        res[kind] = {"outputs_grown": len(outputs), "reps": reps, "disc_mean_rel_gap": gap,
                     **{k + "_ms": v for k, v in med.items()}, **{k + "_ms_min": min(v) for k, v in t.items()},
                     "chain_over_block": med["chain"] / med["block"],
                     "rebuild_over_block": med["rebuild"] / med["block"]}
        print(f"{name:9s} {kind:9s}: rebuild {med['rebuild']:8.3f} ms, chain {med['chain']:8.3f} ms, block "
              f"{med['block']:8.3f} ms (mean gap {gap:.1e})", flush=True)
    return res


def jes_problem(workload, P=10, k=10, seed=0):
    from dkg_amd.jes import compute_sample_box_decomposition

    model, _, _, _ = make_problem(WORKLOADS[workload])
    g = torch.Generator().manual_seed(seed)
    d, m = model.input_dim, model.num_outputs
    sets = [torch.rand(k, d, generator=g, dtype=torch.double) for _ in range(P)]
    fronts = [torch.randn(k, m, generator=g, dtype=torch.double) for _ in range(P)]
    return model, sets, fronts, compute_sample_box_decomposition(fronts)


def measure_jes(workload, reps, warmup):
    from dkg_amd.jes import qLowerBoundMultiObjectiveJointEntropySearch as JES

    model, sets, fronts, bounds = jes_problem(workload)
    t = {"append": [], "refactorise": []}
    fallbacks = 0
    for r in range(warmup + reps):
        for mode in t:
            ms, acq = timed(lambda: JES(model, sets, fronts, bounds, device="cuda:0", conditioning=mode))
            fallbacks = max(fallbacks, acq.append_fallbacks)
            if r >= warmup:
                t[mode].append(ms)
    med = {k: statistics.median(v) for k, v in t.items()}
    print(f"JES construction {workload:9s}: refactorise {med['refactorise']:8.3f} ms, append {med['append']:8.3f} ms",
          flush=True)
    return {"m": model.num_outputs, "n": model.models[0].num_train, "P": len(sets), "k": sets[0].shape[0],
            "reps": reps, "append_fallbacks": fallbacks, **{k + "_ms": v for k, v in med.items()},
            **{k + "_ms_min": min(v) for k, v in t.items()},
            "refactorise_over_append": med["refactorise"] / med["append"]}


def trace(reps):
    """Block updates and single appends at the stress shape alone, for a kernel trace."""
    model, D, upd = cases("stress")
    dev = torch.device("cuda", 0)
    base_model, outputs = upd["decoupled"]
    base = DeviceGPState(base_model, D.to(dev), dev)
    for _ in range(reps):
        block(base, model, outputs)
        m = model.models[0]
        base.with_observation(0, m.train_x[-K], y=m.train_y[-K])
    torch.cuda.synchronize()
    print("done")


def kernel_stats(path):
    out = {}
    for r in csv.DictReader(open(path)):
        for k in KERNELS:
            if k in r["Name"]:
                out[k] = {"avg_us": float(r["AverageNs"]) / 1e3, "calls": int(r["Calls"])}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "append_rows", "bench.json"))
    ap.add_argument("--trace", action="store_true", help="run the stress shape's updates only (for rocprofv3)")
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel-stats CSV of a --trace run to merge into --out")
    a = ap.parse_args()
    if a.kernel_stats:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {}
        res["kernels_stress"] = kernel_stats(a.kernel_stats)
        print(json.dumps(res["kernels_stress"], indent=1))
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench_append_rows.py needs a ROCm device: there is no CPU timing of a GPU path")
        if a.trace:
            return trace(max(a.reps, 20))
        if a.reps < 30 or a.warmup < 5:
            print("note: fewer than 30 repeats / 5 warm-ups: not the documented measurement")
        keep = json.load(open(a.out)).get("kernels_stress") if os.path.exists(a.out) else None
        res = {"kernels_stress": keep} if keep else {}
        res.update(device=torch.cuda.get_device_name(0), timing="synchronised wall time, median")
        for name in SHAPES:
            res[name] = measure(name, a.reps, a.warmup)
        res["jes_construction"] = {k: measure_jes(w, a.reps, a.warmup) for k, w in JES_SHAPES.items()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
