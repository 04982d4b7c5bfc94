"""Timing of the dominated-space box kernels (csrc/dkg_boxes.hip).

Timed, synchronised wall time, medians, the two legs of a shape alternated in the same run:
  hypervolume_front   dkg_amd.boxes.hypervolume_front of one spherical front resident on the device, m = 2 and 3,
                      K = 100, 1000 and 16290 points; the value is read back (a metrics call ends in a float)
  host                dkg_amd.metrics.hypervolume of the same points (the Python recursion), --host-reps each;
                      skipped at m = 3, K = 16290, where one call takes minutes (the result says so)
  dominated_boxes     dkg_amd.boxes.dominated_boxes at the JES preset's 10 samples x 10 points, m = 3, host in and
                      host out, and the device call alone on resident points
Nothing is asserted: the figures are observations.

Writes profiles/boxes/bench.json.
"""

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "decoupled-kg_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
OUT = os.path.join(REPO, "profiles", "boxes", "bench.json")
HOST_SKIP = {(3, 16290)}


def front(K, m, seed=0):
    rng = np.random.default_rng(seed)
    Y = np.abs(rng.normal(size=(K, m))) + 1e-3
    return Y / np.linalg.norm(Y, axis=1, keepdims=True)


def timed(fn, sync):
    if sync:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


def stats(ts):
    return {"median_us": statistics.median(ts), "min_us": min(ts), "reps": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from dkg_amd import metrics
    from dkg_amd.boxes import dominated_boxes, dominated_boxes_device, hypervolume_front

    res = {"shape": "spherical fronts, fp64; device and host legs alternated in one run, medians",
           "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(), "hypervolume": {}}
    for m in (2, 3):
        for K in (100, 1000, 16290):
            Y = front(K, m)
            ref = np.zeros(m)
            Yd = torch.from_numpy(Y).to(DEV)
            dev_leg = lambda: float(hypervolume_front(Yd, ref))  # noqa: E731
            host_leg = lambda: metrics.hypervolume(Y, ref)  # noqa: E731
            for _ in range(a.warmup):
                dev_leg()
            td, th, vd, vh = [], [], None, None
            skip = (m, K) in HOST_SKIP
            for rep in range(a.reps):
                t, vd = timed(dev_leg, True)
                td.append(t)
                if not skip and rep < a.host_reps:
                    t, vh = timed(host_leg, False)
                    th.append(t)
            row = {"device": stats(td), "value": vd}
            if skip:
                row["host"] = "skipped: the host recursion takes minutes at this size"
            else:
                row["host"] = stats(th)
                row["abs_diff"] = abs(vd - vh)
                row["speedup"] = row["host"]["median_us"] / row["device"]["median_us"]
            res["hypervolume"][f"m{m}_K{K}"] = row
            print(f"m={m} K={K}: {row}", flush=True)
    fronts = [torch.from_numpy(front(10, 3, seed=s)) for s in range(10)]
    Yd = torch.stack(fronts).to(DEV)
    legs = {"dominated_boxes_host_in_out": lambda: dominated_boxes(fronts, device=DEV),
            "dominated_boxes_device_call": lambda: dominated_boxes_device(Yd, [-1e10] * 3)}
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    ts = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, fn in legs.items():
            ts[k].append(timed(fn, True)[0])
    res["boxes_10x10_m3"] = {k: stats(v) for k, v in ts.items()}
    res["boxes_10x10_m3"]["J"] = int(dominated_boxes(fronts, device=DEV).shape[2])
    print(res["boxes_10x10_m3"], flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
