"""Per-workgroup phase stamps of the three forward kernels (DKG_DEBUG_STAMPS=1).

Run on the GPU box from the repo root:  python tools/kstamps.py [workload]
Prints, for the last of 20 back-to-back headline forwards: each kernel's
workgroup start/end window on the 100 MHz clock (relative to the first
cross_root start, so the gaps between kernels show), and the per-phase
s_memtime deltas (median / p90 / max over workgroups).

python tools/kstamps.py [workload] --xcd [G ...]  (DKG_DEBUG_STAMPS=3): the envelope launch over G batches
(default 5 and 32), per XCD: first start, last end, workgroups and workgroups with a walked pair (xcd_tables).
"""
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "decoupled-kg_amd")]
XCD = "--xcd" in sys.argv
os.environ["DKG_DEBUG_STAMPS"] = "3" if XCD else "1"
import torch  # noqa: E402

from dkg_amd import DiscreteKnowledgeGradient, _lib  # noqa: E402
from dkg_amd.synthetic import WORKLOADS, make_problem  # noqa: E402


def xcd_tables(wname, batch_counts):
    """python tools/kstamps.py <workload> --xcd 5 32: the envelope launch over G batches (the workload's batch
    repeated, as tools/stage_probe.py launches it) under the two-word stamps of DKG_DEBUG_STAMPS=3, per XCD
    (HW_REG_XCC_ID): first start and last end (us after the launch's first start), workgroups, and workgroups
    with a pair that fails the flat test (from the CPU oracle: tools/env_deal_model.py; the map from workgroup id
    to item is the library's, dkg_debug_envelope_deal).  The last of 6 launches of the stage alone."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from env_deal_model import flat_pairs, walked_workgroups

    w = WORKLOADS[wname]
    model, D, X0, W = make_problem(w)
    acq = DiscreteKnowledgeGradient(model, D, W)
    lib = _lib.load()
    n = 3 * 1024 * 8
    for G in batch_counts:
        plan = acq._state.plan(acq._W, acq._target, G * w.B)
        geo = plan.envelope_geometry()
        walked = walked_workgroups(flat_pairs(w), geo["sw"])
        X = X0.cuda().repeat(G, 1).contiguous()
        plan.time_stage(X, 3, 2)  # the whole forward: the records the envelope reads
        us = plan.time_stage(X, 2, 6) * 1e3
        torch.cuda.synchronize()
        buf = (ctypes.c_ulonglong * n)()
        _lib.check(lib.dkg_debug_read_kstamps(buf, n), "kstamps")
        st = np.frombuffer(buf, dtype=np.uint64).reshape(-1, 2)
        nitems, groups = G * w.B, geo["split"]
        ids = 8 * groups * ((nitems + 7) // 8)
        assert ids <= st.shape[0], f"{ids} workgroups > {st.shape[0]} stamp slots"
        item, member = ctypes.c_int(), ctypes.c_int()
        rows = []  # (xcd, launch residue, start, end, walked)
        for L in range(ids):
            if lib.dkg_debug_envelope_deal(L, nitems, groups, ctypes.byref(item), ctypes.byref(member)) != 1:
                continue
            t0, t1 = int(st[L, 0]), int(st[L, 1])
            rows.append((t1 >> 60, L & 7, t0, t1 & ((1 << 60) - 1), bool(walked[item.value % w.B, member.value])))
        r = np.array(rows, dtype=np.int64)
        base = r[:, 2].min()
        print(f"{wname} x{G}: envelope launch {us:.1f} us (HIP events, mean of 6), {len(rows)} workgroups, "
              f"{int(r[:, 4].sum())} with a walked pair; stamps span {(r[:, 3].max() - base) / 100.0:.1f} us")
        print("  XCD  residues  first start  last end  workgroups  walked   (us after the first start)")
        for x in sorted(set(r[:, 0].tolist())):
            s = r[r[:, 0] == x]
            print(f"  {x:3d}  {sorted(set(s[:, 1].tolist()))!s:>8s}  {(s[:, 2].min() - base) / 100.0:11.2f}"
                  f"  {(s[:, 3].max() - base) / 100.0:8.2f}  {len(s):10d}  {int(s[:, 4].sum()):6d}")
        ends = np.array([(r[r[:, 0] == x][:, 3].max() - base) / 100.0 for x in sorted(set(r[:, 0].tolist()))])
        print(f"  last ends: min {ends.min():.2f}  max {ends.max():.2f}  (max - min) / max {(ends.max() - ends.min()) / ends.max():.2f}")
        del plan


if XCD:
    k = sys.argv.index("--xcd")
    xcd_tables(sys.argv[1] if k > 1 else "headline", [int(a) for a in sys.argv[k + 1:]] or [5, 32])
    sys.exit(0)

w = WORKLOADS[sys.argv[1] if len(sys.argv) > 1 else "headline"]
model, D, X, W = make_problem(w)
acq = DiscreteKnowledgeGradient(model, D, W)
plan = acq._plan_for(w.B)
Xd = X.cuda().contiguous()
kg = torch.empty(w.B, dtype=torch.double, device="cuda")
for _ in range(20):
    plan.forward_into(Xd, kg)
torch.cuda.synchronize()
n = 3 * 1024 * 8
buf = (ctypes.c_ulonglong * n)()
_lib.check(_lib.load().dkg_debug_read_kstamps(buf, n), "kstamps")
st = np.frombuffer(buf, dtype=np.uint64).reshape(3, 1024, 8).astype(np.int64)
nwg = [(w.B + 15) // 16 * ((256 // 16 + 1) // 2) * w.m, ((D.shape[0] + 15) // 16) * ((w.B + 15) // 16) * w.m,
       w.B * plan.state.m and None]
names = ["cross_root", "posterior_cov", "envelope"]
phases = {0: ["plan+prefetch", "stage X", "K fill", "MFMA", "reduce+store"],
          1: ["epi loads", "loads+MFMA", "LDS part", "reduce+store", "-"],
          2: ["issue DMA", "wait+sync", "pairs", "WG sum", "combine"]}
t0 = None
for k in range(3):
    s = st[k]
    used = s[:, 0] > 0
    s = s[used]
    if t0 is None:
        t0 = s[:, 0].min()
    rt0, rt1 = (s[:, 0] - t0) / 100.0, (s[:, 7] - t0) / 100.0  # us
    print(f"{names[k]}: {used.sum()} WGs  start {rt0.min():.2f}..{rt0.max():.2f} us  end {rt1.min():.2f}..{rt1.max():.2f}"
          f" us  (span {rt1.max() - rt0.min():.2f} us)")
    cyc = s[:, 6] - s[:, 1]
    rate = np.median(cyc / np.maximum(1e-9, (s[:, 7] - s[:, 0]) / 100.0))
    print(f"   s_memtime rate ~{rate:.0f} cycles/us; WG lifetime median {np.median(cyc):.0f} mean {cyc.mean():.0f}"
          f" max {cyc.max()} cycles; sum {cyc.sum() / rate:.0f} WG-us = {cyc.sum() / rate / 256:.2f} us on 256 CUs")
    marks = [1, 2, 3, 4, 5, 6]
    for i in range(5):
        a, b = marks[i], marks[i + 1]
        valid = (s[:, a] > 0) & (s[:, b] > 0)
        if valid.sum() == 0:
            continue
        dd = (s[valid, b] - s[valid, a])
        print(f"   {phases[k][i]:>14}: median {np.median(dd):7.0f}  p90 {np.percentile(dd, 90):7.0f}  max {dd.max():7d}")
