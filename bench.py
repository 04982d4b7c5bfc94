"""Discrete-KG throughput on MI355X (BASELINE.json headline metric).

One step = one DiscreteKnowledgeGradient forward over a batch of B candidates
per GPU (the reference's ``forward(X[B,1,d])``, discretekg.py:131-159) at the
headline workload: m=2 outputs, n_train=256, n_disc=1024 (32x32 std grid),
S=16 scalarisations, B=128 candidates per GPU, d=2, fp64.  Inputs and GP state
are resident in HBM before timing.

For N>1 (torchrun, one rank per GPU, RCCL) the default ``--shard
scalarisations`` is the north-star layout (BASELINE.json north_star, SURVEY.md
§8(e)): every rank evaluates the same 128 candidates on its own 16 weight rows
(16*N rows in total, weak scaling) and the per-candidate partial sums meet in
one async RCCL all-reduce per ``--exchange-every`` forward batches (count =
K*B; SURVEY §8(e) amortises the collective over K batches because one small
collective costs about as much host and link latency as a whole forward);
``value`` counts headline-equivalent evals (candidates x 16 scalarisations).
``--shard candidates`` gives every rank its own 128 candidates on all 16 rows and
all-gathers the per-candidate values instead.

A plain run sets up, warms up, times ``--steps`` steps and prints one JSON line (rank 0): value =
KG-evals/s over all ranks, ``ms_per_step`` = the milliseconds one timed step took.  ``--dump-outputs DIR``
also writes the last timed step's per-candidate KG values, as the exchange leaves them, to ``DIR/kg.npy``
(float64; the inputs are seeded, so two runs with the same arguments write the same inputs' values).
Everything else is measured only under ``--full`` (``null`` in a plain line):
  * ``roofline``: the dominant kernel's duration (HIP events on its launch
    stream) against the fp64 roof (78.6 TF/s, vector = matrix on MI355X): ``achieved``
    = SURVEY 8(d)'s counted flops per launch / duration, ``frac`` = achieved / peak;
    ``valu_busy_frac`` (VALU-busy SIMD cycles per launch from the workload's own PMC
    file under profiles/, null when there is none) beside it; every stage in ``stages``;
  * ``cpu_baseline``: a bounded sample of the oracle restatement on the host cores;
  * ``nondegenerate``: the same throughput path on headline sizes with KG > 0 for
    every pair (d = 6; the envelope does real work);
  * ``stress``: the BASELINE configs[4] shape (m 3, n 1024, N 4096, S 32, B 256) in fp64;
  * ``latency_b1``: value+gradient at B = 1, the ``optimize_acqf`` call shape of the
    reference's production loop (bo_loop.py:127-129, batch_limit=1), through
    ``value_and_grad_host`` and through ``forward()`` + autograd on a host X;
  * ``per_rank``: every rank's forward time and its exposed final-collective time.
"""

import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
for _p in (REPO, os.path.join(REPO, "decoupled-kg_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

METRIC = json.load(open(os.path.join(REPO, "BASELINE.json")))["metric"]
# MI355X peaks.  Spec (MI355X_MICROARCH.md / SURVEY 8(d)): 78.6 TF fp64 (vector = matrix), 157.3 TF fp32
# matrix, 8 TB/s HBM.  Measured on the box (tools/ubench/rates.hip, profiles/r02a_rates_f64.txt):
# v_mfma_f64_16x16x4 77.2 TF, v_fma_f64 61.4 TF.
FP64_PEAK_TFLOPS = 78.6
FP64_MFMA_MEASURED_TFLOPS = 77.2
FP64_VALU_MEASURED_TFLOPS = 61.4
FP32_MFMA_PEAK_TFLOPS = 157.3
HBM_PEAK_GBS = 8000.0
SIMDS, CLOCK_GHZ = 1024, 2.4   # 256 CUs x 4 SIMDs
PMC_DIR = os.path.join(REPO, "profiles", "r06")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--workload", default="headline")
    ap.add_argument("--shard", choices=["scalarisations", "candidates"], default="scalarisations",
                    help="axis of the (candidate x scalarisation) space split over ranks (weak scaling)")
    ap.add_argument("--exchange-every", type=int, default=256,
                    help="forward batches per RCCL exchange (count = K*B fp64 values)")
    ap.add_argument("--target", type=int, default=None, help="target_output_ix (decoupled path); default full")
    ap.add_argument("--precision", choices=["fp64", "fp32"], default="fp64",
                    help="fp32: the contractions in fp32 MFMA (DKG_PLAN_F32; BASELINE configs[4], workload stress32)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="bounded CPU-baseline sample (0 = skip)")
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="0: the process's CPU affinity (os.sched_getaffinity), capped by OMP_NUM_THREADS if set")
    ap.add_argument("--profile-reps", type=int, default=50)
    ap.add_argument("--streams", type=int, default=4,
                    help="launches in flight: launch u of an exchange period runs on stream u %% streams with its own "
                         "plan workspace (4: 10.1-10.2 M against 9.1-9.2 M with 2 at --steps 20, 15.8-16.1 M against "
                         "15.4 M at the default; profiles/r05/streams/)")
    ap.add_argument("--batches-per-launch", type=int, default=0,
                    help="forward batches per launch (dkg_plan_forward_batches, bit-identical to one forward per "
                         "batch); 0 = auto: the largest divisor of the exchange period <= min(32, period / streams)")
    ap.add_argument("--graph", type=int, default=2,
                    help="1 = replay each full exchange period (E forwards over the streams) as one captured HIP "
                         "graph; 2 = one single-stream graph per stream per period, replayed side by side")
    ap.add_argument("--graph-head", type=int, default=1,
                    help="--graph 2: each stream's period graph split into its first GRAPH_HEAD forwards and the rest, "
                         "the heads of all streams launched first (0 = one graph per stream)")
    ap.add_argument("--stream-skew", type=int, default=0,
                    help="--graph 2: move this many of the last-launched stream's forwards of a period to the first "
                         "stream (it has work ~3 launches earlier); the results are the same rows either way")
    ap.add_argument("--launch-threads", type=int, default=1,
                    help="--graph 2: host threads enqueuing the streams' graphs side by side (dkg_launcher; "
                         "-1 = one per stream, 1 = the caller alone, in stream order)")
    ap.add_argument("--grad-steps", type=int, default=50, help="timed value+gradient calls at B (0 = skip)")
    ap.add_argument("--b1-calls", type=int, default=200, help="timed value+gradient calls at B = 1 (0 = skip)")
    ap.add_argument("--single-rank-pg", type=int, default=1,
                    help="at one GPU, time the main leg once more with a one-rank RCCL process group, its exchange a "
                         "real all-reduce (the rccl_exchange leg; 0 = skip)")
    ap.add_argument("--nd-steps", type=int, default=256,
                    help="timed steps of the non-degenerate headline-size leg (workload headline_nd; 0 = skip)")
    ap.add_argument("--pmc", default="auto",
                    help="per-kernel PMC figures per launch (tools/pmc_passes.sh + tools/pmc_report.py); auto: "
                         "profiles/r05/pmc_<workload>[_fp32].json, none if that file does not exist")
    ap.add_argument("--prep-reps", type=int, default=5, help="timed device-state preparations (0 = skip)")
    ap.add_argument("--stress32-steps", type=int, default=16,
                    help="timed forwards of the stress32 leg (BASELINE configs[4] as specified: fp32 contractions, "
                         "against the fp64 plan of the same workload; 0 = skip)")
    ap.add_argument("--stress-streams", type=int, default=2,
                    help="launch streams of the stress legs (each its own plan; eager launches): one forward's stage "
                         "tails overlap the next one's (16 steps: 1 stream 724-731 K, 2 streams 786-814 K, 4 775-778 K "
                         "KG-evals/s; profiles/r05/stress_streams/)")
    ap.add_argument("--stress-steps", type=int, default=16,
                    help="timed forwards of the stress leg (BASELINE configs[4] shape, fp64; 0 = skip)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline's timed steps also run every other leg (single-stream run, per-kernel "
                         "rooflines, batch diagnostics, value+gradient, B = 1 latency, state preparation, "
                         "non-degenerate, stress and stress32 legs, the one-rank RCCL exchange, the CPU baseline); "
                         "without it the line holds the headline's figures and null for the rest")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last timed step handed its caller as DIR/<name>.npy "
                         "(kg.npy: the per-candidate KG values, float64)")
    args = ap.parse_args()
    if not args.full:
        # a plain run: set up, warm up, time the steps, print the line; every leg with a run of its own is off
        args.cpu_seconds = 0.0
        args.grad_steps = args.b1_calls = args.prep_reps = 0
        args.nd_steps = args.stress_steps = args.stress32_steps = 0
        args.single_rank_pg = 0
    return args


def last_step_outputs(tp, steps):
    """What the timed path handed its caller for its last step: the per-candidate KG values of step
    ``steps - 1`` after the exchange (world 1: the forward's own row; scalarisations sharded: the mean over
    every rank's weight rows, [B]; candidates sharded: every rank's candidates, [world, B])."""
    x = tp.xchg
    slot, r = x._slot(steps - 1)
    if x.mode == "gather":
        rows = x.rows[slot]
        kg = x.gathered[slot][:x.world * rows * x.B].view(x.world, rows, x.B)[:, r]
    else:
        kg = x.bufs[slot][r]
        if x.collective:  # the buffer holds the sum over ranks of S_local * (the rank's mean)
            kg = kg / (x.S_local * x.world)
    return {"kg": kg.detach().to("cpu", torch.double).contiguous()}


def dump_outputs(outdir, arrays):
    os.makedirs(outdir, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(outdir, f"{name}.npy"), t.numpy())


def stage_model(w, m, n, N, B, S, d):
    """Algorithmic flops / HBM bytes per launch of each kernel."""
    kev = 3 * d + 8  # flops per kernel evaluation (distance + Matern profile)
    fl_cross = sum(B * nn * (nn + 1) + 2 * B * nn + B * nn * kev for nn in n)
    fl_cov = sum(2 * B * N * nn + B * N * kev for nn in n)
    fl_env = B * S * (N + 1) * (4 * m + 2)
    by_cross = sum(8 * (nn * nn + nn * d + B * nn + B) for nn in n) + 8 * B * d
    by_cov = sum(8 * (B * nn + N * nn + B * N) for nn in n) + 8 * (B + N) * d
    by_env = 8 * (m * (N + B * N + B) + S * m + B)
    return {"cross_root_kernel": (fl_cross, by_cross), "posterior_cov_kernel": (fl_cov, by_cov),
            "envelope_kernel": (fl_env, by_env)}


def survey_model(m, n, N, S, B, d):
    """SURVEY.md 8(d) / BASELINE.md algorithmic cost of one forward of B candidates (fp64):
    F = B * (sum_i [2 n_i^2 + 2 n_i N + (3d+8)(n_i+N+1)] + S (N+1)(5m+1)),
    Bytes = 8 [sum_i (n_i^2 + n_i N + N + n_i d) + N d + B d + S m + B]."""
    f_eval = sum(2 * nn * nn + 2 * nn * N + (3 * d + 8) * (nn + N + 1) for nn in n) + S * (N + 1) * (5 * m + 1)
    by = 8 * (sum(nn * nn + nn * N + N + nn * d for nn in n) + N * d + B * d + S * m + B)
    return f_eval * B, by


def cpu_info(requested: int):
    aff = len(os.sched_getaffinity(0))
    threads = requested or aff
    omp = os.environ.get("OMP_NUM_THREADS")
    if not requested and omp and omp.isdigit():
        threads = min(threads, int(omp))   # the GPU box's CPU share (OMP_NUM_THREADS=16 there)
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return threads, aff, model


def cpu_baseline(model, D, W, X, target, seconds, threads_req):
    """The oracle's structure-faithful restatement of the reference path on host cores."""
    from oracle.discretekg import calculate_discrete_kg, calculate_discrete_kg_conditioning_on_single_output
    from oracle.gp import ModelList, OutputGP

    threads, aff, cpu_model = cpu_info(threads_req)
    torch.set_num_threads(threads)
    om = ModelList([OutputGP(m.train_x, m.train_y, m.lengthscale, m.outputscale, m.noise, m.mean_constant,
                             m.kernel, m.nu, m.y_mean, m.y_std) for m in model.models])
    Xc = X.cpu()

    def one(x):
        if target is None:
            return calculate_discrete_kg(om, x, D, W)
        return calculate_discrete_kg_conditioning_on_single_output(om, x, target, D, W)

    one(Xc[0])  # warm-up (builds the per-model caches, as GPyTorch does on first call)
    t0 = time.perf_counter()
    cnt = 0
    while time.perf_counter() - t0 < seconds or cnt < 4:
        one(Xc[cnt % Xc.shape[0]])
        cnt += 1
    dt = time.perf_counter() - t0
    return {"value": cnt / dt, "unit": "KG-evals/s", "cores": threads, "kind": "port",
            "cpu_model": cpu_model, "affinity_cpus": aff,
            # BASELINE.md's plan names len(sched_getaffinity) threads; on the GPU box that is the whole host, of
            # which one GPU's share is OMP_NUM_THREADS (16), so the sample runs there and this is the linear
            # upper bound of the same restatement on every CPU of the affinity set (it scales sublinearly)
            "value_at_affinity_linear_upper_bound": cnt / dt * aff / max(1, threads),
            "sample": f"{cnt} forwards cycling over the {Xc.shape[0]} headline candidates (per-candidate loop, "
                      f"dense (N+1)^2 posterior covariance, reference epigraph walk; torch fp64 CPU, "
                      f"{threads} threads), {dt:.1f} s"}


def hip_runtime():
    """The HIP runtime instance torch already loaded (hipGraphLaunch for the per-stream graph replays): opened
    by the path it is mapped from, so no second copy of the runtime is loaded."""
    path = "libamdhip64.so.7"
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line and line.strip().split()[-1].startswith("/"):
                path = line.strip().split()[-1]
                break
    lib = ctypes.CDLL(path)
    for name, args in (("hipGraphLaunch", [ctypes.c_void_p, ctypes.c_void_p]),
                       ("hipEventCreateWithFlags", [ctypes.c_void_p, ctypes.c_uint]),
                       ("hipEventRecord", [ctypes.c_void_p, ctypes.c_void_p]),
                       ("hipStreamWaitEvent", [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint])):
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = ctypes.c_int
    return lib


def hip_check(rc: int, what: str) -> None:
    if rc:
        raise RuntimeError(f"{what} failed: HIP error {rc}")


_SIDE_STREAMS = []


def side_streams(dev, n):
    """The launch streams besides the current one, created once and shared by every leg: HIP maps streams onto
    the process's hardware queues (GPU_MAX_HW_QUEUES = 4) in creation order, so streams created afresh for a
    later leg could land on the current stream's queue and serialise with it (a two-stream stress leg then ran
    at the one-stream rate on some runs)."""
    while len(_SIDE_STREAMS) < n:
        _SIDE_STREAMS.append(torch.cuda.Stream(dev))
    return _SIDE_STREAMS[:n]


class Throughput:
    """The timed throughput path: E forward batches per exchange, ``G`` batches per launch
    (``dkg_plan_forward_batches``: one launch per stage runs G forwards, each its own B candidates and its
    own result row, bit for bit what G ``forward_into`` calls write), the launches of a period dealt over
    ``streams`` HIP streams with one captured HIP graph per stream (DESIGN.md §6 "Forward batches in flight")."""

    def __init__(self, acq, X, B, E, mode, S_local, dev, precision, G=1):
        from dkg_amd.dist import BatchExchange

        self.acq, self.B, self.E, self.dev = acq, B, E, dev
        self.G = max(1, min(G, E))
        if E % self.G:
            raise ValueError(f"--batches-per-launch {G} does not divide the exchange period {E}")
        self.plan = acq._plan_for(B)
        self.Xd = X.to(dev).contiguous()
        # every batch of a launch is the workload's B candidates (as every step of earlier rounds was)
        self.XG = self.Xd.repeat(self.G, 1).contiguous()
        self.xchg = BatchExchange(B, E, mode, S_local=S_local, device=dev)
        self.main = torch.cuda.current_stream(dev)
        self.f32 = precision == "fp32"
        self.head = 0
        self.launch_threads = -1
        self.skew = 0
        self.want_breakdown = False  # --full: one more, untimed, replay of a one-period region with event marks

    def chunks(self, k0, k1, G):
        """(first step, batches, unit index in its period) of the launches covering steps k0 .. k1 - 1:
        G batches each, cut at exchange-period ends."""
        k = k0
        while k < k1:
            g = min(G, k1 - k, self.E - k % self.E)
            yield k, g, (k % self.E) // G
            k += g

    def run(self, ns, steps, warmup, graph, world, G=None):
        E, xchg, main_s, dev, B = self.E, self.xchg, self.main, self.dev, self.B
        G = self.G if G is None else G
        streams = [main_s] + side_streams(dev, ns - 1)
        plans = [self.acq._state.plan(self.acq._W, self.acq._target, G * B, f32=self.f32) for _ in range(ns)]
        XG = self.XG

        def join():
            for s in streams[1:]:
                main_s.wait_stream(s)

        def launch(k, g, i, kg):
            if g == 1:
                plans[i].forward_into(self.Xd, kg)
            else:
                plans[i].forward_batches_into(XG[:g * B], kg, B)

        def unit(k, g, u):
            kg = xchg.block(k, g)
            if ns > 1 and k % E == 0:
                for s in streams[1:]:
                    s.wait_stream(main_s)
            with torch.cuda.stream(streams[u % ns]):
                launch(k, g, u % ns, kg)
            if (k + g) % E == 0:
                join()
            xchg.done(k + g - 1)

        for k, g, u in self.chunks(0, warmup, G):
            unit(k, g, u)
        join()
        xchg.flush(warmup)
        torch.cuda.synchronize()
        nunits = E // G
        graphs = []
        launcher = None
        if graph == 2 and steps >= E:
            # per stream one single-stream graph of its units u = i mod ns: replayed on its own stream, each
            # enqueues its launches as one batch (a graph forked over streams replays node by node);
            # each stream's units in two pieces, its first `head` units and the rest: the heads of all
            # streams are launched first, so every stream has work a few us into the period instead of
            # after the launches of the whole graphs before it (a launch costs ~1 us of host per kernel)
            own = [list(range(i, nunits, ns)) for i in range(ns)]
            kk = max(0, min(self.skew, len(own[-1]) - 1)) if ns > 1 else 0
            if kk:  # `skew` units of the last stream moved to the first
                own[0] += own[-1][len(own[-1]) - kk:]
                own[-1] = own[-1][:len(own[-1]) - kk]
            for slot in range(2):
                gs = []
                for i in range(ns):
                    rows = own[i]
                    parts = [rows[:self.head], rows[self.head:]] if 0 < self.head < len(rows) else [rows]
                    pieces = []
                    for part in parts:
                        g_ = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g_, stream=streams[i] if i else torch.cuda.Stream(dev),
                                              capture_error_mode="thread_local"):
                            for u in part:
                                launch(u * G, G, i, xchg.bufs[slot][u * G:(u + 1) * G].view(-1))
                        pieces.append(g_)
                    gs.append(pieces)
                graphs.append(gs)
            torch.cuda.synchronize()
            # replayed with hipGraphLaunch on the raw executable graphs (what CUDAGraph.replay calls, without
            # its Python and stream-guard overhead: ~9 instead of ~18 us of host time per launch)
            hip = hip_runtime()
            execs = [[[ctypes.c_void_p(g_.raw_cuda_graph_exec()) for g_ in pieces] for pieces in gs] for gs in graphs]
            npieces = max(len(p) for gs in graphs for p in gs)
            sptrs = [ctypes.c_void_p(s.cuda_stream) for s in streams]
            nthr = ns if self.launch_threads < 0 else max(1, min(ns, self.launch_threads))
            if nthr > 1:
                from dkg_amd.launch import GraphLauncher

                launcher = GraphLauncher(nthr)
                for slot in range(2):
                    launcher.prepare(slot, [s.cuda_stream for s in streams],
                                     [[g_.value for g_ in pieces] for pieces in execs[slot]])
            # the fork / join events, created once (torch's wait_stream creates an event per call)
            evs = [ctypes.c_void_p() for _ in range(ns)]
            for e in evs:
                hip_check(hip.hipEventCreateWithFlags(ctypes.byref(e), 2), "hipEventCreateWithFlags")  # no timing
        elif graph and steps >= E:
            # one graph per exchange buffer: the period's launches forked over the streams exactly as the eager
            # path does; replayed on the main stream, so the collective after it orders as before
            for slot in range(2):
                g_ = torch.cuda.CUDAGraph()
                # thread_local: the RCCL watchdog thread may query events while this thread captures
                with torch.cuda.graph(g_, capture_error_mode="thread_local"):
                    cs = torch.cuda.current_stream(dev)
                    lanes = [cs] + streams[1:]
                    for s in lanes[1:]:
                        s.wait_stream(cs)
                    for u in range(nunits):
                        with torch.cuda.stream(lanes[u % ns]):
                            launch(u * G, G, u % ns, xchg.bufs[slot][u * G:(u + 1) * G].view(-1))
                    for s in lanes[1:]:
                        cs.wait_stream(s)
                graphs.append(g_)
            torch.cuda.synchronize()
        if graphs:
            # one untimed replay of every graph (the first launch of a graph uploads it)
            for g_ in graphs:
                for gi in (g_ if isinstance(g_, list) else [g_]):
                    for gp in (gi if isinstance(gi, list) else [gi]):
                        gp.replay()
            torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        if graphs and graph == 2 and launcher is not None:
            launcher.arm(5.0 + 1e-4 * steps)  # workers spin through the timed region
        # every event of the region made before its clock starts (creating one costs host time)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        evc = torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        ev0.record()
        if not graphs:
            for s in streams[1:]:
                s.wait_stream(main_s)
        k0 = 0
        host = 0.0  # host seconds inside the launch calls (replay / plan launches)
        if graphs:
            while k0 + E <= steps:
                xchg.block(k0, 1)
                th = time.perf_counter()
                g_ = graphs[(k0 // E) % 2]
                if graph == 2:
                    # fork: every stream after the main stream's work so far (the previous period's exchange);
                    # the first period starts on an idle device (synchronized above), so it needs none
                    if k0 > 0:
                        hip_check(hip.hipEventRecord(evs[0], sptrs[0]), "hipEventRecord")
                        for i in range(1, ns):
                            hip_check(hip.hipStreamWaitEvent(sptrs[i], evs[0], 0), "hipStreamWaitEvent")
                    if launcher is not None:
                        launcher.launch((k0 // E) % 2)
                    else:
                        for p in range(npieces):
                            for i, pieces in enumerate(execs[(k0 // E) % 2]):
                                if p < len(pieces):
                                    hip_check(hip.hipGraphLaunch(pieces[p], sptrs[i]), "hipGraphLaunch")
                    for i in range(1, ns):
                        hip_check(hip.hipEventRecord(evs[i], sptrs[i]), "hipEventRecord")
                        hip_check(hip.hipStreamWaitEvent(sptrs[0], evs[i], 0), "hipStreamWaitEvent")
                else:
                    g_.replay()
                host += time.perf_counter() - th
                xchg.done(k0 + E - 1)
                k0 += E
        if k0 < steps:  # steps past the last whole period (or no graphs): eager launches
            for k, g, u in self.chunks(k0, steps, G):
                th = time.perf_counter()
                unit(k, g, u)
                host += time.perf_counter() - th
            join()
        # (a whole-period region ended with every stream's join event on the main stream: no join needed)
        evc.record()  # every forward of the timed region enqueued before this point on the main stream
        xchg.flush(steps)
        ev1.record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        self.host_us_per_step = host / max(1, steps) * 1e6
        if graphs and graph == 2 and launcher is not None:
            launcher.arm(0.0)
            launcher.close()
        self.breakdown = None
        if self.want_breakdown and graphs and graph == 2 and launcher is None and steps == E:
            # where a one-period region's time goes: the same launches again, untimed, with an event on every
            # stream after each of its pieces and the host clock after each hipGraphLaunch; GPU times relative
            # to an event on the main stream just before the first launch
            torch.cuda.synchronize()
            e_start = torch.cuda.Event(enable_timing=True)
            marks = [[torch.cuda.Event(enable_timing=True) for _ in range(npieces)] for _ in range(ns)]
            e_start.record(streams[0])
            launch_us = []
            th0 = time.perf_counter()
            for p in range(npieces):
                for i, pieces in enumerate(execs[0]):
                    if p < len(pieces):
                        hip_check(hip.hipGraphLaunch(pieces[p], sptrs[i]), "hipGraphLaunch")
                        launch_us.append(round((time.perf_counter() - th0) * 1e6, 1))
                        marks[i][p].record(streams[i])
            torch.cuda.synchronize()
            wall_us = (time.perf_counter() - th0) * 1e6
            done = [[round(e_start.elapsed_time(marks[i][p]) * 1e3, 1) for p in range(npieces)
                     if p < len(execs[0][i])] for i in range(ns)]
            self.breakdown = {
                "what": "an untimed replay of the timed region's launches (steps == E: one period), per stream "
                        "the GPU time at which each piece (its first `head` launches, then the rest) had finished, "
                        "and the host time after each hipGraphLaunch, both from just before the first launch",
                "forwards_per_stream": [len(p) * G for p in own], "batches_per_launch": G,
                "host_launch_done_us": launch_us, "stream_piece_done_us": done,
                "last_stream_done_us": max(d[-1] for d in done), "wall_us": round(wall_us, 1)}
        # this rank's device time of the forwards, and what the last exchange adds after them (exposed)
        self.compute_ms = ev0.elapsed_time(evc)
        self.exposed_ms = evc.elapsed_time(ev1)
        if world > 1:
            dist.barrier()
        gpu_s = ev0.elapsed_time(ev1) / 1e3
        t = torch.tensor([max(wall, gpu_s)], dtype=torch.double, device=dev)
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t)


def batch_stats(plan, Xd):
    """SURVEY.md 8(d) diagnostics of one batch: short-circuit rate, KG distribution, envelope sizes."""
    kg_s, pairs_s, hull_s = plan.forward_stats(Xd)
    pairs_c, hull_c, kg_c = pairs_s.cpu(), hull_s.cpu().long(), kg_s.cpu()
    hist = torch.bincount(hull_c.reshape(-1)).tolist()
    return {"pairs": int(pairs_c.numel()),
            "short_circuit_frac": float((hull_c == 1).double().mean()),
            "zero_kg_frac": float((pairs_c == 0).double().mean()),
            "envelope_lines_mean": float(hull_c.double().mean()),
            "envelope_lines_hist": {str(h): c for h, c in enumerate(hist) if c},
            "kg_quantiles": {str(q): float(torch.quantile(kg_c, q)) for q in (0.0, 0.1, 0.5, 0.9, 1.0)}}


def stage_rooflines(plan, Xd, model_fb, reps, precision, pmc, G=1, B=None):
    """Every forward kernel, as the timed region launches it (G forward batches of B candidates per launch:
    ``plan`` holds G * B, ``Xd`` the G batches), against the compute roof (fp64 78.6 TF/s; the fp32 MFMA peak
    for fp32 contractions) with its counted flops, and against HBM with its algorithmic bytes (``model_fb``:
    stage_model of the whole launch).  Durations: HIP events around `reps` back-to-back launches of the
    kernel alone on its own stream (dkg_plan_time_stage_batches).  VALU-busy and traffic come from the
    workload's PMC file when there is one (else null)."""
    names = ["cross_root_kernel", "posterior_cov_kernel", "envelope_kernel"]
    if G > 1:
        avg_ms = [plan.time_stage_batches(Xd, B, k, reps) for k in range(3)]
    else:
        avg_ms = [plan.time_stage(Xd, k, reps) for k in range(3)]
    out = {}
    for i, name in enumerate(names):
        fl, by = model_fb[name]
        t = avg_ms[i] * 1e-3
        p = pmc.get(name, {})
        peak = FP32_MFMA_PEAK_TFLOPS if (precision == "fp32" and name != "envelope_kernel") else FP64_PEAK_TFLOPS
        ach = fl / t / 1e12
        busy = p.get("valu_busy_simd_cycles")
        r = {"avg_launch_us": t * 1e6, "algorithmic_flops": fl, "algorithmic_bytes": by,
             "bound": STAGE_BOUND[name], "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak,
             "hbm_gbs_algorithmic": by / t / 1e9, "hbm_frac": by / t / 1e9 / HBM_PEAK_GBS,
             "traffic": p.get("hbm_bytes_per_launch"),
             "valu_busy_frac": (busy / t / (SIMDS * CLOCK_GHZ * 1e9)) if busy else None,
             "mfma_busy_frac_pmc": p.get("mfma_busy_frac"),
             "valu_insts_per_wave": p.get("valu_insts_per_wave")}
        out[name] = r
    return out


# What limits each stage (measured: kstamps / PMC): the two contractions run on the fp64 MFMA; the envelope is
# fp64 VALU issue and dependent latency (reductions, LDS round trips, the walk's serial steps), priced against
# the fp64 vector peak, which is the same 78.6 TF/s on MI355X.
STAGE_BOUND = {"cross_root_kernel": "mfma", "posterior_cov_kernel": "mfma", "envelope_kernel": "valu/latency"}


def batches_per_launch(E: int, args) -> int:
    """Forward batches per launch: --batches-per-launch, or the largest divisor of the exchange period E
    that leaves every stream a launch of its own (E / streams) and is at most 32 (a 32-batch launch of the
    headline already fills the device many times over: 8,192 envelope workgroups)."""
    if args.batches_per_launch > 0:
        # an explicit G applies to every leg; a leg whose exchange period it does not divide (e.g. headline_nd's
        # E = 256 under --batches-per-launch 5) takes the largest divisor of its E below it
        return max(g for g in range(1, min(args.batches_per_launch, E) + 1) if E % g == 0)
    cap = max(1, min(32, E // max(1, args.streams)))
    return max(g for g in range(1, cap + 1) if E % g == 0)


def pmc_file(args) -> str:
    if args.pmc != "auto":
        return args.pmc
    return os.path.join(PMC_DIR, f"pmc_{args.workload}{'_fp32' if args.precision == 'fp32' else ''}.json")


def main():
    args = parse()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # DKG_BENCH_BACKEND=gloo: rehearsal of the N > 1 path with several ranks on one GPU (not a bench line)
    backend = os.environ.get("DKG_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local %= max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # the launch streams before any process group: HIP deals its hardware queues (GPU_MAX_HW_QUEUES = 4 on the box)
    # to streams in creation order
    side_streams(dev, max(args.streams, args.stress_streams, 1) - 1)
    pg_file = None
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from dkg_amd import DiscreteKnowledgeGradient
    from dkg_amd.synthetic import WORKLOADS, make_problem
    from dkg_amd.utils import sample_simplex

    def setup(wname, G=None, precision=None, steps=None):
        """The workload's plan and throughput driver; `steps`: the leg's own step count, which sets its exchange
        period (the headline's --steps for the main line)."""
        precision = precision or args.precision
        w = WORKLOADS[wname]
        model, D, X0, W = make_problem(w)
        X = X0
        if args.shard == "candidates":
            # weak scaling: every rank evaluates its own B candidates (Sobol stream per rank)
            if rank > 0:
                X = torch.quasirandom.SobolEngine(w.d, scramble=True, seed=4 + 1000 * rank).draw(w.B, dtype=torch.double)
            W_local = W
        else:
            # weak scaling: S rows per rank out of S*world rows of one qMC simplex sample, dealt round robin
            # (rank r takes rows r, r + world, ...), so every rank's rows spread over the simplex alike and
            # the ranks' flat / walked pair mixes match statistically (per_rank.batch_stats shows them); at
            # world = 1 this is the workload's W itself (the same sample_simplex draw)
            W_all = W if world == 1 else sample_simplex(w.m, w.S * world, qmc=True, seed=11, dtype=torch.double)
            W_local = W_all[rank::world].contiguous()
        acq = DiscreteKnowledgeGradient(model, D, W_local, target_output_ix=args.target, device=dev,
                                        precision=precision)
        E = max(1, min(args.exchange_every, steps or args.steps))
        tp = Throughput(acq, X, w.B, E, "gather" if args.shard == "candidates" else "reduce", w.S, dev,
                        precision, G=batches_per_launch(E, args) if G is None else G)
        tp.head = args.graph_head
        tp.launch_threads = args.launch_threads
        tp.skew = args.stream_skew
        tp.want_breakdown = args.full
        return w, model, D, X0, W, acq, tp

    w, model, D, X0, W, acq, tp = setup(args.workload)
    single = None
    if args.full and (args.streams > 1 or args.graph):
        e1 = tp.run(1, args.steps, args.warmup, False, world, G=1)
        single = {"value": world * w.B * args.steps / e1, "ms_per_step": e1 / args.steps * 1e3}
    elapsed = tp.run(max(1, args.streams), args.steps, args.warmup, args.graph, world)
    value = world * w.B * args.steps / elapsed
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_step_outputs(tp, args.steps))
    mine = torch.tensor([tp.compute_ms, tp.exposed_ms, elapsed * 1e3], dtype=torch.double, device=dev)
    if world > 1:
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
    else:
        allr = [mine]
    per_rank = {"compute_ms": [float(r[0]) for r in allr], "exposed_collective_ms": [float(r[1]) for r in allr],
                "elapsed_ms": [float(r[2]) for r in allr],
                "what": "compute: HIP events from the start of the timed region to the last forward enqueued; "
                        "exposed: from there to the end of the final exchange (the collective nothing overlaps); "
                        "batch_stats: each rank's own pairs (its weight rows x its candidates)"}

    # ---- --full: per-kernel rooflines; the dominant kernel's is the line's `roofline`
    roof = None
    if args.full:
        pmc = {}
        pmc_path = pmc_file(args)
        if os.path.exists(pmc_path):
            try:
                pmc = json.load(open(pmc_path))
            except (OSError, ValueError):
                pmc = {}
        # the stages as the timed region launches them: G batches per launch
        G = tp.G
        model_fb = stage_model(w, w.m, [mm.num_train for mm in model.models], D.shape[0], G * w.B, w.S, w.d)
        gplan_roof = acq._state.plan(acq._W, acq._target, G * w.B, f32=args.precision == "fp32")
        stages = stage_rooflines(gplan_roof, tp.XG, model_fb, args.profile_reps, args.precision, pmc, G=G, B=w.B)
        del gplan_roof
        dom = max(stages, key=lambda k: stages[k]["avg_launch_us"])
        roof = dict(stages[dom], kernel=dom,
                    bound_note="fp64 compute roof: 78.6 TF/s is both the vector and the matrix fp64 peak of MI355X; "
                               "achieved = SURVEY 8(d) counted flops per launch / launch duration; the envelope is "
                               "VALU-issue and latency bound (its comparisons, selects and reductions are not counted "
                               "flops): valu_busy_frac is its occupancy figure",
                    stages={k: {kk: v[kk] for kk in ("avg_launch_us", "bound", "frac", "valu_busy_frac", "traffic")}
                            for k, v in stages.items()},
                    launch=f"{G} forward batch(es) of {w.B} candidates per launch, as in the timed region",
                    pmc_source=os.path.relpath(pmc_path, REPO) if pmc else None)

    # ---- whole-forward roofline as BASELINE.md defines it: max(F/P, Bytes/BW) / T_measured
    f_fwd, b_fwd = survey_model(w.m, [mm.num_train for mm in model.models], D.shape[0], w.S, w.B, w.d)
    t_fwd = elapsed / args.steps
    t_min = max(f_fwd / (FP64_PEAK_TFLOPS * 1e12), b_fwd / (HBM_PEAK_GBS * 1e9))
    fwd_roof = {"definition": "BASELINE.md: max(F/P_fp64, Bytes/BW_HBM) / T_forward", "flops": f_fwd,
                "bytes": b_fwd, "t_min_us": t_min * 1e6, "t_forward_us": t_fwd * 1e6, "frac": t_min / t_fwd}
    # ---- --full: the batch's diagnostics (one forward_stats launch)
    stats = None
    if args.full:
        stats = batch_stats(tp.plan, tp.Xd)
        # every rank's pair mix (the work a weak-scaling rank does depends on how many of its pairs walk an envelope)
        mine_st = torch.tensor([stats["zero_kg_frac"], stats["short_circuit_frac"], stats["envelope_lines_mean"],
                                (1.0 - stats["zero_kg_frac"]) * stats["pairs"]], dtype=torch.double, device=dev)
        if world > 1:
            all_st = [torch.zeros_like(mine_st) for _ in range(world)]
            dist.all_gather(all_st, mine_st)
        else:
            all_st = [mine_st]
        per_rank["batch_stats"] = {"zero_kg_frac": [float(r[0]) for r in all_st],
                                   "short_circuit_frac": [float(r[1]) for r in all_st],
                                   "envelope_lines_mean": [float(r[2]) for r in all_st],
                                   "pairs_with_kg_above_0": [int(round(float(r[3]))) for r in all_st]}

    # ---- value + gradient (dkg_plan_forward_grad: the optimize_acqf L-BFGS-B path), same batch
    grad_info = None
    lat_b1 = None
    if args.precision == "fp64":
        if args.grad_steps > 0:
            gplan = acq._plan_for(w.B, grad=True)
            for _ in range(3):
                gplan.forward_grad(tp.Xd)
            torch.cuda.synchronize()
            g0 = time.perf_counter()
            for _ in range(args.grad_steps):
                gplan.forward_grad(tp.Xd)
            torch.cuda.synchronize()
            gdt = (time.perf_counter() - g0) / args.grad_steps
            grad_info = {"value": w.B / gdt, "unit": "KG-evals+gradients/s (per GPU)", "ms_per_step": gdt * 1e3}
        if args.b1_calls > 0:
            # B = 1: the reference's production call shape (bo_loop.py:127-129), one synchronous C call
            # per L-BFGS-B evaluation; the host needs the value and gradient back each time
            # value_and_grad_host: host x in, host (KG, dKG/dx) out, one round trip
            p1 = acq._plan_for(1, grad=True)
            xh = tp.Xd.cpu()
            for i in range(5):
                p1.forward_grad(tp.Xd[:1].contiguous())
                acq.value_and_grad_host(xh[i:i + 1])
            torch.cuda.synchronize()
            ts, te, ta = [], [], []
            for i in range(5):  # the autograd route's plans and pinned buffers
                xa = xh[i:i + 1].unsqueeze(-2).requires_grad_(True)
                torch.autograd.grad(-acq(xa).sum(), xa)
            for i in range(args.b1_calls):
                x1 = xh[i % w.B:i % w.B + 1]
                t0 = time.perf_counter()
                acq.value_and_grad_host(x1)
                ts.append(time.perf_counter() - t0)
                xd = tp.Xd[i % w.B:i % w.B + 1].contiguous()
                t0 = time.perf_counter()
                kg1, g1 = p1.forward_grad(xd)
                kg1.cpu(), g1.cpu()
                te.append(time.perf_counter() - t0)
                # what gen_candidates_scipy does per L-BFGS-B evaluation: a host X[1, 1, d] with requires_grad,
                # the acquisition's forward, autograd back to X (bo_loop.py:127-129 -> optimize_acqf)
                t0 = time.perf_counter()
                xa = x1.unsqueeze(-2).requires_grad_(True)
                loss = -acq(xa).sum()
                (ga,) = torch.autograd.grad(loss, xa)
                float(loss.detach()), ga.numpy()
                ta.append(time.perf_counter() - t0)
            ts.sort()
            te.sort()
            ta.sort()
            lat_b1 = {"median_us": ts[len(ts) // 2] * 1e6, "p90_us": ts[int(len(ts) * 0.9)] * 1e6,
                      "calls": len(ts), "eager_two_copies_median_us": te[len(te) // 2] * 1e6,
                      "autograd_route": {"median_us": ta[len(ta) // 2] * 1e6, "p90_us": ta[int(len(ta) * 0.9)] * 1e6,
                                         "what": "host X[1, 1, d].requires_grad_() -> acq(X) -> autograd.grad "
                                                 "(the unchanged optimize_acqf call; _HostForwardFn: one round "
                                                 "trip, host backward)"},
                      "what": "value + dKG/dx at one host candidate through the public entry the L-BFGS-B "
                              "objective calls (value_and_grad_host: model check, pinned H2D, 3 launches, one "
                              "pinned D2H), device round trip included; eager_two_copies: the plan's C call on a "
                              "device candidate + two .cpu() copies"}

    # ---- state preparation: what a refit costs before the first forward (DeviceGPState: per output the
    # kernel matrix, Cholesky with the psd_safe_cholesky jitter check, the inverse, alpha, Q_D and mu_D)
    prep = None
    if args.prep_reps > 0:
        from dkg_amd.gp_state import DeviceGPState

        DeviceGPState(model, D, dev)
        torch.cuda.synchronize()
        tp_ = []
        for _ in range(args.prep_reps):
            t0 = time.perf_counter()
            DeviceGPState(model, D, dev)
            torch.cuda.synchronize()
            tp_.append(time.perf_counter() - t0)
        tp_.sort()
        prep = {"ms_median": tp_[len(tp_) // 2] * 1e3, "ms_min": tp_[0] * 1e3, "outputs": w.m, "reps": len(tp_),
                "what": "DeviceGPState(model, D) on the host clock, synchronised: every output's caches"}

    # ---- non-degenerate leg: headline sizes, KG > 0 for every pair (workload headline_nd, d = 6)
    nd = None
    if args.nd_steps > 0 and args.workload == "headline" and args.precision == "fp64":
        wn, _, Dn, _, _, _, tpn = setup("headline_nd", steps=args.nd_steps)
        en = tpn.run(max(1, args.streams), args.nd_steps, min(args.warmup, 10), args.graph, world)
        env_us = tpn.plan.time_stage(tpn.Xd, 2, args.profile_reps) * 1e3
        nd = {"workload": "headline_nd", "value": world * wn.B * args.nd_steps / en, "unit": "KG-evals/s",
              "steps": args.nd_steps, "ms_per_step": en / args.nd_steps * 1e3, "envelope_us": env_us,
              "config": {"m": wn.m, "n_train": wn.n_train, "n_disc": Dn.shape[0], "S": wn.S, "B": wn.B, "d": wn.d,
                         "lengthscales": wn.lengthscales, "outputscales": wn.outputscales, "noise": wn.noise},
              "batch_stats": batch_stats(tpn.plan, tpn.Xd)}

    # ---- stress leg: BASELINE configs[4]'s shape (m 3, n 1024, N 4096, S 32, B 256), fp64
    stress = None
    if args.stress_steps > 0 and args.workload == "headline" and args.precision == "fp64":
        ws, ms, Ds, _, _, _, tps = setup("stress", G=1)
        es = tps.run(max(1, args.stress_streams), args.stress_steps, 2, False, world)
        fb = stage_model(ws, ws.m, [mm.num_train for mm in ms.models], Ds.shape[0], ws.B, ws.S, ws.d)
        # the stress workload's own PMC file (profiles/r05/pmc_stress.json) for its stages' traffic / busy figures
        pmc_s_path = os.path.join(PMC_DIR, "pmc_stress.json")
        pmc_s = json.load(open(pmc_s_path)) if os.path.exists(pmc_s_path) else {}
        st_s = stage_rooflines(tps.plan, tps.Xd, fb, 3, "fp64", pmc_s)
        stress = {"workload": "stress", "value": world * ws.B * args.stress_steps / es, "unit": "KG-evals/s",
                  "steps": args.stress_steps, "streams": max(1, args.stress_streams),
                  "ms_per_step": es / args.stress_steps * 1e3, "dtype": "f64",
                  "config": {"m": ws.m, "n_train": ws.n_train, "n_disc": Ds.shape[0], "S": ws.S, "B": ws.B,
                             "d": ws.d},
                  "stages": {k: {kk: v[kk] for kk in ("avg_launch_us", "achieved", "frac", "traffic", "valu_busy_frac",
                                                      "mfma_busy_frac_pmc")} for k, v in st_s.items()},
                  "pmc_source": os.path.relpath(pmc_s_path, REPO) if pmc_s else None}
        del tps

    # ---- stress32 leg: BASELINE configs[4] as specified (fp32 contractions, noise 1e-3 of the outputscale),
    # timed next to the fp64 plan of the same workload; the fp32 error against fp64 on the same candidates
    stress32 = None
    if args.stress32_steps > 0 and args.workload == "headline" and args.precision == "fp64":
        legs, kgs = {}, {}
        for prec in ("fp64", "fp32"):
            w3, m3, D3, _, _, _, tp3 = setup("stress32", G=1, precision=prec)
            e3 = tp3.run(max(1, args.stress_streams), args.stress32_steps, 2, False, world)
            fb3 = stage_model(w3, w3.m, [mm.num_train for mm in m3.models], D3.shape[0], w3.B, w3.S, w3.d)
            pmc3_path = os.path.join(PMC_DIR, f"pmc_stress32{'_fp32' if prec == 'fp32' else ''}.json")
            pmc3 = json.load(open(pmc3_path)) if os.path.exists(pmc3_path) else {}
            st3 = stage_rooflines(tp3.plan, tp3.Xd, fb3, 3, prec, pmc3)
            kg3 = torch.empty(w3.B, dtype=torch.double, device=dev)
            tp3.plan.forward_into(tp3.Xd, kg3)
            kgs[prec] = kg3.cpu()
            legs[prec] = {"value": world * w3.B * args.stress32_steps / e3,
                          "ms_per_step": e3 / args.stress32_steps * 1e3,
                          "stages": {k: {kk: v[kk] for kk in ("avg_launch_us", "achieved", "peak", "frac", "traffic",
                                                              "mfma_busy_frac_pmc")} for k, v in st3.items()},
                          "pmc_source": os.path.relpath(pmc3_path, REPO) if pmc3 else None}
            del tp3
        k64, k32 = kgs["fp64"], kgs["fp32"]
        keep = k64.abs() >= 1e-3 * k64.abs().max()
        rel = ((k32 - k64).abs() / k64.abs())[keep]
        v32, v64 = legs["fp32"]["value"], legs["fp64"]["value"]
        stress32 = {"workload": "stress32", "value": v32, "unit": "KG-evals/s", "steps": args.stress32_steps,
                    "streams": max(1, args.stress_streams),
                    "dtype": "f32 contractions (MFMA, peak 157.3 TF/s) / f64 envelope",
                    "ms_per_step": legs["fp32"]["ms_per_step"], "stages": legs["fp32"]["stages"],
                    "pmc_source": legs["fp32"]["pmc_source"], "fp64_same_workload": legs["fp64"],
                    "fp32_beats_fp64": v32 > v64, "fp32_over_fp64": v32 / v64,
                    "error_vs_fp64": {"candidates_kg_above_1e-3_max": int(keep.sum()),
                                      "max_rel": float(rel.max()) if rel.numel() else None,
                                      "median_rel": float(rel.median()) if rel.numel() else None,
                                      "frac_within_rel_1e-3": float((rel <= 1e-3).double().mean())
                                      if rel.numel() else None},
                    "note": "SURVEY 8(d) asks rel 1e-3 against fp64; at this conditioning (cancellation factor "
                            "c ~ 1e3..6e4) fp32 contractions leave ~c 1e-6 relative slope error, so rel 1e-3 is "
                            "out of reach (DESIGN.md 4.6); tests/test_gpu_parity.py::test_f32_stress32_error_model "
                            "holds every candidate to that error model instead"}

    # ---- the exchange through RCCL at one GPU: a one-rank communicator (FileStore under /tmp, no rendezvous) made
    # after every other leg, and the main leg timed again with it, so the exchange after every period is the real
    # RCCL all-reduce an N-GPU rank makes and exposed_collective_ms measures it.  Kept out of `value`: with a
    # process group alive the launch path measured ~10 % slower at --steps 20 (torch's RCCL watchdog thread
    # polls the work events; profiles/r06/bench/pg_ab.txt), which is a cost of N > 1 runs, not of one GPU.
    rccl_leg = None
    if world == 1 and args.single_rank_pg and backend == "nccl":
        import tempfile

        fd, pg_file = tempfile.mkstemp(prefix="dkg_pg1_", dir="/tmp")
        os.close(fd)
        os.unlink(pg_file)
        dist.init_process_group("nccl", store=dist.FileStore(pg_file, 1), rank=0, world_size=1, device_id=dev)
        _, _, _, _, _, _, tpr = setup(args.workload)
        er = tpr.run(max(1, args.streams), args.steps, args.warmup, args.graph, 1)
        rccl_leg = {"value": w.B * args.steps / er, "unit": "KG-evals/s", "ms_per_step": er / args.steps * 1e3,
                    "compute_ms": tpr.compute_ms, "exposed_collective_ms": tpr.exposed_ms,
                    "exposed_frac": tpr.exposed_ms / (er * 1e3),
                    "what": "the main leg again with a one-rank RCCL (nccl) process group: the exchange of every "
                            f"{tpr.E}-batch period is a real RCCL all-reduce of {tpr.E} x {w.B} fp64 values; "
                            "exposed = the final exchange nothing overlaps (what an N-GPU rank waits for at the end "
                            "of this region)"}

    out = None
    if rank == 0:
        cpu = None
        if args.cpu_seconds > 0 and world == 1:
            cpu = cpu_baseline(model, D, W, X0, args.target, args.cpu_seconds, args.cpu_threads)
        E = tp.E
        out = {
            "metric": METRIC,
            "value": value,
            "unit": "KG-evals/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64" if args.precision == "fp64" else "f32 contractions / f64 envelope",
            "data": f"synthetic: seeded GP-prior draw, lengthscales family ({w.lengthscales}, s={w.outputscales}, "
                    f"noise {'%g x s' % w.noise_rel if w.noise_rel > 0 else w.noise})",
            "config": {"workload": args.workload, "m": w.m, "n_train": w.n_train, "n_disc": D.shape[0],
                       "S": w.S, "B_per_gpu": w.B, "d": w.d,
                       "path": "full" if args.target is None else f"target_output_ix={args.target}",
                       "shard": args.shard,
                       "parallelism": f"{args.shard} sharded over {world} GPU(s); one async RCCL "
                                      f"{'all-gather' if args.shard == 'candidates' else 'all-reduce'} "
                                      f"per {E} forward batches",
                       "exchange_every": E, "streams": max(1, args.streams),
                       "batches_per_launch": tp.G,
                       "launch": f"{tp.G} forward batch(es) of {w.B} candidates per launch of each stage "
                                 "(dkg_plan_forward_batches: each batch its own candidates and result row, the "
                                 "same bits as one forward per batch)",
                       "hip_graph": {0: "off", 1: "one graph forked over the streams",
                                     2: "one single-stream graph per stream"}.get(args.graph, str(args.graph))
                       + (f" (first {args.graph_head} forward(s) of every stream launched first)"
                          if args.graph == 2 and args.graph_head > 0 else "")
                       + (f", enqueued by {max(1, args.streams) if args.launch_threads < 0 else args.launch_threads}"
                          " host thread(s) side by side (dkg_launcher)" if args.graph == 2 else "")},
            "host_launch_us_per_step": tp.host_us_per_step,
            "region_breakdown": getattr(tp, "breakdown", None),
            "single_stream": single,
            "forward_calls_per_s": world * args.steps / elapsed,
            "value_and_grad": grad_info,
            "latency_b1": lat_b1,
            "state_prep": prep,
            "roofline": roof,
            "forward_roofline": fwd_roof,
            "batch_stats": stats,
            "nondegenerate": nd,
            "stress": stress,
            "stress32": stress32,
            "per_rank": per_rank,
            "rccl_exchange": rccl_leg,
            "cpu_baseline": cpu,
        }
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
    if dist.is_initialized():
        dist.destroy_process_group()
    if pg_file and os.path.exists(pg_file):
        os.unlink(pg_file)


if __name__ == "__main__":
    main()
