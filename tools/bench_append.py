"""Appending an observation to the device GP state against rebuilding it.

Two ways to the device state of the n + 1 model, timed in one process, alternating, synchronised wall
time, median of --reps repeats after --warmup warm-ups:
  rebuild : DeviceGPState(model) -- every output's Cholesky, inverse, alpha, root_frag, Q_D, mu_D
  append  : state_n.with_observation(...) -- the bordered update of the grown outputs only
at the headline shape (m = 2, 255 -> 256, N = 1024) and the stress shape (m = 3, 1023 -> 1024, N = 4096),
each for a decoupled update (output 0 grows) and a full update (every output grows).

    python tools/bench_append.py                       # timings -> profiles/append/bench_append.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_append.py --trace stress
    python tools/bench_append.py --kernel-stats DIR/.../run_kernel_stats.csv    # adds the per-kernel times

The discretisation kernel (append_disc_kernel) is memory-bound: its bytes are the old disc_frag read and the
new one written, N_pad (n_pad(n) + n_pad(n + 1)) 8, and its rate is given against the HBM peak.
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

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E specification
HBM_COPY_GBS = 6290.0      # measured float4 copy rate on the same part
SHAPES = ("headline", "stress")


def pad16(x):
    return (x + 15) // 16 * 16


def head(st, n):
    return SingleTaskGPState(st.train_x[:n], st.train_y[:n], st.lengthscale, st.outputscale, st.noise,
                             st.mean_constant, st.kernel, st.nu, st.y_mean, st.y_std)


def cases(name):
    """(model of n + 1, D, {update: (model of n, grown outputs)})."""
    model, D, _, _ = make_problem(WORKLOADS[name])
    n1 = model.models[0].num_train
    dec = ModelListGPState(*[head(m, n1 - 1) if i == 0 else m for i, m in enumerate(model.models)])
    full = ModelListGPState(*[head(m, n1 - 1) for m in model.models])
    return model, D, {"decoupled": (dec, [0]), "full": (full, list(range(model.num_outputs)))}


def grow(state, model, outputs):
    for i in outputs:
        m = model.models[i]
        state = state.with_observation(i, m.train_x[-1], y=m.train_y[-1])
    return state


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def measure(name, reps, warmup):
    model, D, upd = cases(name)
    dev = torch.device("cuda", 0)
    Dd = D.to(dev)
    res = {"m": model.num_outputs, "n": model.models[0].num_train - 1, "N": D.shape[0]}
    for kind, (base_model, outputs) in upd.items():
        base = DeviceGPState(base_model, Dd, dev)
        t_build, t_app = [], []
        for r in range(warmup + reps):
            tb, cold = timed(lambda: DeviceGPState(model, Dd, dev))
            ta, warm = timed(lambda: grow(base, model, outputs))
            if r >= warmup:
                t_build.append(tb)
                t_app.append(ta)
        # the two states describe the same model: the appended means against the rebuilt ones
        gap = max(float((a.disc_mean - b.disc_mean).abs().max() / b.disc_mean.abs().max())
                  for a, b in zip(warm.outputs, cold.outputs))
        mb, ma = statistics.median(t_build), statistics.median(t_app)
        res[kind] = {"outputs_grown": len(outputs), "rebuild_ms": mb, "append_ms": ma, "ratio": mb / ma,
                     "rebuild_ms_min": min(t_build), "append_ms_min": min(t_app), "reps": reps,
                     "disc_mean_rel_gap": gap}
        print(f"{name:9s} {kind:9s}: rebuild {mb:8.3f} ms, append {ma:8.3f} ms, ratio {mb / ma:6.2f} "
              f"(mean gap {gap:.1e})", flush=True)
    return res


def trace(name, reps):
    """Appends alone, for a kernel trace."""
    model, D, upd = cases(name)
    dev = torch.device("cuda", 0)
    base_model, outputs = upd["decoupled"]
    base = DeviceGPState(base_model, D.to(dev), dev)
    for _ in range(reps):
        grow(base, model, outputs)
    torch.cuda.synchronize()
    print("done")


def kernel_stats(path, name):
    """Average time per append kernel from a rocprofv3 kernel-stats CSV, and the discretisation kernel's rate."""
    w = WORKLOADS[name]
    n, N = w.n_train - 1, w.n_disc
    out = {}
    for r in csv.DictReader(open(path)):
        for k in ("append_copy_kernel", "append_solve_kernel", "append_disc_kernel", "pack_linv_kernel"):
            if k in r["Name"]:
                out[k] = {"avg_us": float(r["AverageNs"]) / 1e3, "calls": int(r["Calls"])}
    if "append_disc_kernel" in out:
        nbytes = pad16(N) * (pad16(n) + pad16(n + 1)) * 8
        gbs = nbytes / (out["append_disc_kernel"]["avg_us"] * 1e-6) / 1e9
        out["append_disc_kernel"].update(bytes=nbytes, GBs=gbs, of_hbm_peak=gbs / HBM_PEAK_GBS,
                                         of_hbm_copy_rate=gbs / HBM_COPY_GBS)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "append", "bench_append.json"))
    ap.add_argument("--trace", choices=SHAPES, help="run appends of this shape only (for rocprofv3)")
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel-stats CSV of a --trace run to merge into --out")
    ap.add_argument("--stats-shape", choices=SHAPES, default="stress")
    a = ap.parse_args()
    if a.kernel_stats:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {}
        res.setdefault("kernels", {})[a.stats_shape] = kernel_stats(a.kernel_stats, a.stats_shape)
        print(json.dumps(res["kernels"][a.stats_shape], indent=1))
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench_append.py needs a ROCm device: there is no CPU timing of a GPU path")
        if a.trace:
            return trace(a.trace, max(a.reps, 20))
        if a.reps < 30 or a.warmup < 5:
            print("note: fewer than 30 repeats / 5 warm-ups: not the documented measurement")
        res = json.load(open(a.out)).get("kernels") if os.path.exists(a.out) else None
        res = {"kernels": res} if res else {}
        res.update(device=torch.cuda.get_device_name(0), timing="synchronised wall time, median",
                   hbm_peak_GBs=HBM_PEAK_GBS)
        for name in SHAPES:
            res[name] = measure(name, a.reps, a.warmup)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
