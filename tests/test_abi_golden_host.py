"""The host side of the core C entries (csrc/dkg_abi.hip, csrc/dkg_launch.hip), pinned to a recording: workspace
sizes, the host-only value queries, every refusal that needs no device and the calls that return DKG_OK without
work (no GPU: a size query launches nothing, and every recorded call returns before its first HIP call, as the
other ``*_host`` tests rely on).

``tests/golden/abi_host.json`` holds, for every entry of ``queries()``, the value at each argument tuple in order, and
for every call of ``calls()`` in order its ``(status, dkg_last_error())`` (the labels stay here).  It was recorded
from the build of the commit before the one that put the plan workspace on one carve and the core ABI on
dkg_kernels.h's error helpers, with that build's library in ``DKG_LIB``, from the repository root:

    import json, sys
    sys.path[:0] = ["tests", "decoupled-kg_amd"]
    import test_abi_golden_host as t
    json.dump(t.record(), open("tests/golden/abi_host.json", "w"), separators=(",", ":"))

The test replays both lists and compares for equality: a byte of a message, a status, the order of two checks or a
byte of a workspace that moves fails it.

How each call stays on the host.  A plan initialisation is given a zero-byte workspace, and the workspace check is
the last one before build_plan writes the plan, so a call that passes every other check ends there (its message
carries the required total); none reaches copy_disc_means.  The one-shot forward, the preparations, the MLL and the
append check their workspace last as well.  The entries that take a plan are given a hand-written host plan (``Plan``
below mirrors csrc/dkg_kernels.h; its size is checked against dkg_plan_bytes()) whose fields lead into a refusal or
the B = 0 return.  DKG_DEBUG_STAMPS and DKG_ENV_SW must be unset: the first allocates on the device, the second
changes the envelope geometry the sizes depend on.
"""

import ctypes
import itertools
import json
import os
from ctypes import c_double, c_int, c_int32, c_int64, c_size_t, c_uint64, c_void_p

FAKE = 64  # a pointer that is never followed: the checks come first
GRAD, F32, FUSED, GROWS, FORCE = 1, 4, 8, 32, 128
ENV_REGIONS = 20  # include/dkg.h DKG_ENV_LDS_REGIONS


def _lib():
    from dkg_amd import _lib as L

    return L


class Plan(ctypes.Structure):
    """``struct Plan`` (csrc/dkg_kernels.h), for the entries that read a host plan's fields before anything else."""


def _plan_fields():
    P8 = c_void_p * 8
    return [("o", _lib().DkgOutput * 8)] + [(k, c_int32) for k in (
        "m", "d", "N", "S", "target", "max_B", "max_np", "sw", "split", "debug_env", "debug_cov", "debug_stamp", "grad",
        "bpad", "stream", "f32")] + [("disc", c_void_p), ("weights", c_void_p)] + [(k, P8) for k in (
            "q", "kx", "mux", "var", "jq", "qxrm", "qdrm", "gmu")] + [(k, c_void_p) for k in (
                "kstamps", "mux_all", "var_all", "cov_all", "mu_all")] + [("cov_stride", c_int64)] + [
                    (k, c_void_p) for k in ("wg_part", "tickets", "dup", "wg_gpart")] + [
                        (k, P8) for k in ("q32", "root32", "disc32")] + [
                            ("hull_pairs", c_void_p), ("fused", c_int32), ("sync", c_void_p), ("sync_err", c_void_p),
                            ("sync_bytes", c_size_t), ("icpt", c_void_p), ("icpt_stride", c_int32), ("itop", c_void_p),
                            ("itopk", c_void_p), ("kx32", P8), ("ntgt", c_int32), ("tlist", c_int32 * 9),
                            ("tpack", c_uint64), ("grad_rows", c_int32)]


def _plan(**fields):
    if not hasattr(Plan, "m"):
        Plan._fields_ = _plan_fields()
    assert ctypes.sizeof(Plan) == _lib().load().dkg_plan_bytes()
    p = Plan()
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _outs(ns, at=None):
    """Outputs of fake pointers with ns[i] training points; at: {index: {field: value}}."""
    outs = (_lib().DkgOutput * max(len(ns), 1))()
    for o, n in zip(outs, ns):
        o.n, o.kernel, o.outputscale, o.noise, o.y_std = n, 2, 1.0, 1e-2, 1.0
        for f in ("inv_lengthscale", "train_x", "alpha", "root_frag", "disc_frag", "disc_mean"):
            setattr(o, f, FAKE)
    for i, fields in (at or {}).items():
        for k, v in fields.items():
            setattr(outs[i], k, v)
    return outs


# ragged training sizes per output count; n >= 512 turns the K(x, X) fill on by size
NS = [(37,), (512,), (5, 256), (1, 1024), (37, 5, 1), (256, 512, 37), (1, 5, 37, 256, 512, 1024, 5, 37),
      (37, 5, 1, 256, 37, 5, 1, 256)]
_N = (0, 1, 2111, 2112, 5000)  # N + 1 <= 64 * 33 holds at 2111 and fails at 2112: the intercept scratch
_B = (0, 1, 17, 511, 512)  # KFILL_MIN_B = 512
_S = (1, 8, 9, 17, 64)  # envelope split 1, 1, 2, 3, 8: wg_part / wg_gpart exist above 1
_D = (1, 3, 16)
_FLAGS = (0, GRAD, F32, GRAD | GROWS, GRAD | FORCE)
_T = (0, 1, 2)  # index into (1, 2, m + 1)


def _thin(axes, p):
    """Every p-th tuple of the axes' product (p a prime that divides no axis length, so no axis is skipped over)."""
    return [row for k, row in enumerate(itertools.product(*axes)) if k % p == 0]


def _fill(ns, B):
    return max(ns) >= 497 or B >= 512


FORWARD_GRID = _thin((NS, _N, _B, _S), 7)
PLAN_GRID = _thin((NS, _D, _N, _B, _S, _FLAGS), 113)
TARGETS_GRID = [(ns, d, N, B, S, (1, 2, len(ns) + 1)[t], f) for ns, d, N, B, S, t, f in
                _thin((NS, _D, _N, _B, _S, _T, _FLAGS), 331)]
# (m, d, n, N, S): both sides of the staged gradient rows' LDS limit (tests/test_grad_rows_host.py)
ROWS_SHAPES = [(2, 2, 256, 1024, 16), (2, 2, 1024, 121, 16), (2, 6, 640, 64, 8), (2, 6, 800, 64, 8),
               (3, 2, 1024, 4096, 32), (3, 2, 1024, 50, 32), (8, 16, 128, 50, 8), (8, 16, 256, 50, 8), (1, 1, 16, 10,
                   1)]
ROWS_FLAGS = (GRAD, GRAD | GROWS, GRAD | FORCE, GRAD | GROWS | FORCE, 0, F32, GRAD | F32, GROWS, GRAD | 64)
# (m, N, waves, S, d, max_np, grad, stream, grows)
ENV_LDS = [(1, 0, 1, 1, 1, 16, 0, 0, 0), (2, 1024, 8, 16, 2, 256, 0, 0, 0), (2, 1024, 8, 16, 2, 256, 1, 0, 0),
           (3, 5000, 8, 17, 3, 48, 0, 1, 0), (3, 50, 8, 32, 2, 1024, 1, 1, 1), (8, 50, 8, 8, 16, 256, 1, 1, 0),
           (8, 2111, 1, 64, 16, 1024, 0, 0, 0)]


def queries():
    """entry -> [thunk]: the size and value queries, in the fixture's order."""
    lib = _lib().load()
    q = {}

    def size(name, *args):
        q.setdefault(name, []).append(lambda: int(getattr(lib, name)(*args)))

    for ns, N, B, S in FORWARD_GRID:
        size("dkg_forward_workspace", _outs(ns), len(ns), N, B, S)
    for ns, d, N, B, S, f in PLAN_GRID:
        size("dkg_plan_workspace", _outs(ns), len(ns), d, N, B, S, f)
    for ns, d, N, B, S, T, f in TARGETS_GRID:
        size("dkg_plan_workspace_targets", _outs(ns), len(ns), d, N, B, S, T, f)
    three = _outs((37, 36, 35))
    for outs, m in ((None, 3), (three, 0), (_outs((5,) * 9), 9)):  # the zero-returning cases
        size("dkg_forward_workspace", outs, m, 50, 17, 3)
        size("dkg_plan_workspace", outs, m, 3, 50, 17, 3, 0)
        size("dkg_plan_workspace_targets", outs, m, 3, 50, 17, 3, 1, 0)
    for T in (0, 5, -1):
        size("dkg_plan_workspace_targets", three, 3, 3, 50, 17, 3, T, 0)
    for n in (0, -1, 1, 5, 16, 37, 256, 1000, 1024, 1025):
        size("dkg_prepare_workspace", n)
    for ns in [(n,) for n in (1, 16, 31, 32, 33, 37, 1000, 1024, 0, 1025)] + [
            (37, 36, 16), (1, 1024), (1, 5, 37, 256, 512, 1024, 5, 37), (37, 0, 5), (5, 1025), (5,) * 9]:
        size("dkg_mll_workspace", (c_int * len(ns))(*ns), len(ns))
    size("dkg_mll_workspace", None, 1)
    size("dkg_mll_workspace", (c_int * 1)(5), 0)
    for n, N in ((1, 0), (37, 50), (1023, 1 << 22), (1024, 5), (0, 5), (5, -1)):
        size("dkg_append_workspace", n, N)
    for rows, n in ((0, 0), (1, 1), (16, 16), (17, 37), (50, 1024), (-3, 5), (5, -3), (4096, 1000)):
        size("dkg_frag_elems", rows, n)
    size("dkg_plan_bytes")
    for m, d, n, N, S in ROWS_SHAPES:
        for f in ROWS_FLAGS:
            size("dkg_plan_grad_rows", _outs((n,) * m), m, d, N, S, f)

    def env_lds(*a):
        out = (c_int * (ENV_REGIONS + 1))()
        return [int(lib.dkg_debug_envelope_lds(*a, out))] + list(out)

    for name, field in (("dkg_plan_fused", "fused"), ("dkg_plan_grad_rows_of", "grad_rows")):
        size(name, None)
        size(name, ctypes.byref(_plan()))
        size(name, ctypes.byref(_plan(**{field: 1})))
    q["dkg_debug_envelope_lds"] = [lambda a=a: env_lds(*a) for a in ENV_LDS]
    return q


def calls():
    """[(label, thunk)]: every thunk is a call that returns before any device work, refused or with nothing to do."""
    L = _lib()
    lib = L.load()
    out = []

    def add(label, fn, *args):
        out.append((label, lambda: fn(*args)))

    three = (37, 36, 35)
    host = ctypes.create_string_buffer(lib.dkg_plan_bytes())

    # ---- the plan: (outs, m, d, disc, N, weights, S, target, max_B, flags, ws, bytes, host, dev, stream)
    def init(label, ns=three, at=None, m=None, d=3, disc=FAKE, N=50, w=FAKE, S=3, target=-1, max_B=4, flags=0, ws=FAKE,
             nbytes=0, h=host, dev=FAKE, null_outs=False):
        o = None if null_outs else _outs(ns, at)
        add("plan_init " + label, lib.dkg_plan_init, o, len(ns) if m is None else m, d, disc, N, w, S, target, max_B,
            flags, ws, nbytes, h, dev, None)

    def init_t(label, targets, T=None, ns=three, d=3, N=50, w=FAKE, S=3, max_B=4, flags=0, nbytes=0, h=host):
        t = None if targets is None else (c_int * len(targets))(*targets)
        add("plan_init_targets " + label, lib.dkg_plan_init_targets, _outs(ns), len(ns), d, FAKE, N, w, S, t,
            len(targets or ()) if T is None else T, max_B, flags, FAKE, nbytes, h, FAKE, None)

    init("NULL host plan", h=None)
    init("NULL device plan", dev=None)
    init("NULL outs", null_outs=True)
    for label, kw in (("m=0", {"m": 0}), ("m=9", {"m": 9, "ns": (5,) * 9}), ("d=0", {"d": 0}), ("d=17", {"d": 17}),
                      ("m=9 d=17", {"m": 9, "ns": (5,) * 9, "d": 17}), ("max_B=-1", {"max_B": -1}), ("N=-1", {"N": -1}),
                      ("S=0", {"S": 0}), ("target=m", {"target": 3}), ("target=-2", {"target": -2}),
                      ("N=2^22+1", {"N": (1 << 22) + 1}), ("S=2^20 m=3", {"S": 1 << 20}),
                      ("S=2^20 with NULL weights", {"S": 1 << 20, "w": None}), ("NULL weights", {"w": None}),
                      ("NULL workspace", {"ws": None}), ("NULL disc", {"disc": None}),
                      ("NULL disc at N=0 is fine", {"disc": None, "N": 0}), ("flags=64", {"flags": 64}),
                      ("flags=64 with a short workspace", {"flags": GRAD | 64, "nbytes": 255}),
                      ("GROWS without GRAD", {"flags": GROWS}), ("FORCE without GRAD", {"flags": FORCE}),
                      ("GRAD | F32", {"flags": GRAD | F32}), ("GRAD | F32 | FORCE", {"flags": GRAD | F32 | FORCE}),
                      ("S=0 with flags=64", {"S": 0, "flags": 64})):
        init(label, **kw)
    for label, fields in (("n=0", {"n": 0}), ("n=1025", {"n": 1025}), ("n=1009 pads to 1024", {"n": 1009}),
                          ("kernel id 4", {"kernel": 4}), ("kernel id -1", {"kernel": -1}),
                          ("NULL lengthscale", {"inv_lengthscale": None}), ("NULL train_x", {"train_x": None}),
                          ("NULL alpha", {"alpha": None}), ("NULL root", {"root_frag": None}),
                          ("NULL disc_frag", {"disc_frag": None}), ("NULL disc_mean", {"disc_mean": None})):
        init("output 1 " + label, at={1: fields})
    init("output 1 NULL disc_frag at N=0 is fine", at={1: {"disc_frag": None}}, N=0)
    init("output 0 n=0 before output 1 kernel id", at={0: {"n": 0}, 1: {"kernel": 7}})
    init("output 2 n=1024 d=16", ns=(37, 36, 1024), d=16)
    # the workspace check, the last one: the required total at each kind of plan
    for m, d, n, N, S in ROWS_SHAPES:
        for f in (F32, GRAD) + ((GRAD | GROWS, GRAD | FORCE) if n == 800 else ()):
            init(f"m{m} d{d} n{n} N{N} S{S} flags {f}", ns=(n,) * m, d=d, N=N, S=S, flags=f)
    for f in (0, GRAD):
        for N, S, B in ((0, 1, 0), (2111, 9, 17), (2112, 17, 512), (50, 64, 511)):
            init(f"ragged N{N} S{S} B{B} flags {f}", ns=(37, 512, 5), N=N, S=S, max_B=B, flags=f, nbytes=4096)
    init_t("NULL host plan", [0], h=None)
    init_t("NULL targets", None, T=1)
    for label, t, T in (("T=0", [0], 0), ("T=m+2", [0, 1, 2, -1, 0], 5), ("repeated targets with T=m+2", [0, 0, 0, 0,
        0], 5),
                        ("targets[1]=m", [0, 3], None), ("targets[0]=-2", [-2], None), ("repeat", [1, -1, 1], None)):
        init_t(label, t, T)
    init_t("FUSED with T=2", [0, 1], flags=FUSED)
    init_t("FUSED with T=1 is fine", [1], flags=FUSED)
    init_t("FUSED with T=2 and repeated targets", [1, 1], flags=FUSED)
    init_t("S=0 before the targets", [7], S=0)
    for T, f in ((2, 0), (4, GRAD), (4, F32)):
        for S, B in ((3, 4), (9, 17), (17, 512)):
            init_t(f"T{T} S{S} B{B} flags {f}", [-1, 0, 1, 2][:T], S=S, max_B=B, flags=f)

    # dkg_plan_grad_rows' own refusals (its shapes are in queries())
    def rows(label, ns=three, m=None, d=3, N=50, S=3, flags=GRAD, at=None, null_outs=False):
        add("plan_grad_rows " + label, lib.dkg_plan_grad_rows, None if null_outs else _outs(ns, at),
            len(ns) if m is None else m, d, N, S, flags)

    rows("NULL outs", null_outs=True)
    for label, kw in (("m=9 d=17", {"m": 9, "ns": (5,) * 9, "d": 17}), ("N=-1", {"N": -1}), ("S=0", {"S": 0}),
                      ("N=-1 S=0", {"N": -1, "S": 0}), ("N=2^22+1", {"N": (1 << 22) + 1}), ("S=2^20", {"S": 1 << 20}),
                      ("S=2^20 flags=64", {"S": 1 << 20, "flags": 64}), ("flags=0", {"flags": 0}),
                      ("flags=F32", {"flags": F32}), ("output 1 n=0", {"at": {1: {"n": 0}}})):
        rows(label, **kw)

    # ---- the one-shot forward: (outs, m, d, disc, N, x, B, weights, S, target, kg, pairs, ws, bytes, stream)
    def forward(label, ns=three, at=None, m=None, d=3, N=50, x=FAKE, B=1, w=FAKE, S=3, target=-1, kg=FAKE, nbytes=0):
        add("forward " + label, lib.dkg_forward, _outs(ns, at), len(ns) if m is None else m, d, FAKE, N, x, B, w, S,
            target,
            kg, None, FAKE, nbytes, None)

    forward("B=0 returns at once", B=0)
    forward("B=0 still checks the outputs", B=0, at={2: {"kernel": 9}})
    forward("B=0 d=17", B=0, d=17)
    forward("B=-1", B=-1)
    forward("short workspace")
    forward("short workspace, one byte over the plan slot", nbytes=lib.dkg_plan_bytes() + 512)
    forward("m=8 ragged", ns=NS[6], N=2112, B=17, S=9)
    forward("NULL weights", w=None)
    forward("target=3", target=3)
    add("forward_timed NULL stage_ms", lib.dkg_forward_timed, _outs(three), 3, 3, FAKE, 50, FAKE, 1, FAKE, 3, -1, FAKE,
        None, FAKE, 0, None, None)
    ms = (ctypes.c_float * 3)()
    add("forward_timed B=0", lib.dkg_forward_timed, _outs(three), 3, 3, FAKE, 50, FAKE, 0, FAKE, 3, -1, FAKE, None,
        FAKE,
        0, None, ms)
    add("forward_timed short workspace", lib.dkg_forward_timed, _outs(three), 3, 3, FAKE, 50, FAKE, 1, FAKE, 3, -1,
        FAKE,
        None, FAKE, 0, None, ms)

    # ---- the entries that take a plan
    blank, cap4 = _plan(), _plan(m=3, d=3, N=50, S=3, max_B=4, ntgt=1)
    grad4 = _plan(m=3, d=3, N=50, S=3, max_B=4, ntgt=1, grad=1)
    grad16 = _plan(m=3, d=16, N=50, S=3, max_B=8, ntgt=1, grad=1)
    two = _plan(m=3, d=3, N=0, S=1, max_B=4, ntgt=2)
    f32p = _plan(m=2, d=3, N=50, S=3, max_B=4, ntgt=1, f32=1)
    ref = ctypes.byref
    add("plan_forward NULL host plan", lib.dkg_plan_forward, None, FAKE, FAKE, 1, FAKE, None, None)
    add("plan_forward NULL device plan", lib.dkg_plan_forward, ref(blank), None, FAKE, 1, FAKE, None, None)
    for label, p, x, B, kg in (("blank B=-1", blank, FAKE, -1, FAKE), ("blank B=0", blank, FAKE, 0, FAKE),
                               ("blank B=0 NULL data", blank, None, 0, None), ("blank B=1", blank, FAKE, 1, FAKE),
                               ("B=5 of 4", cap4, FAKE, 5, FAKE), ("B=5 of 4 NULL x", cap4, None, 5, FAKE),
                               ("NULL x", cap4, None, 1, FAKE), ("NULL kg", cap4, FAKE, 4, None)):
        add("plan_forward " + label, lib.dkg_plan_forward, ref(p), FAKE, x, B, kg, None, None)
        add("plan_forward_timed " + label, lib.dkg_plan_forward_timed, ref(p), FAKE, x, B, kg, None, None, ms)
    add("plan_forward_timed NULL stage_ms", lib.dkg_plan_forward_timed, ref(cap4), FAKE, FAKE, 1, FAKE, None, None,
        None)
    add("plan_forward_batches NULL plan", lib.dkg_plan_forward_batches, None, FAKE, FAKE, 1, 1, FAKE, None)
    for label, p, x, B, nb, kg in (("two targets", two, FAKE, 1, 1, FAKE), ("two targets B=-1", two, FAKE, -1, 1, FAKE),
                                   ("B=-1", cap4, FAKE, -1, 1, FAKE), ("nbatch=-1", cap4, FAKE, 1, -1, FAKE),
                                   ("B=0", cap4, FAKE, 0, 5, FAKE), ("nbatch=0", cap4, None, 5, 0, None),
                                   ("blank B=0", blank, FAKE, 0, 0, FAKE), ("3 x 2 of 4", cap4, FAKE, 2, 3, FAKE),
                                   ("2^16 x 2^16", cap4, FAKE, 1 << 16, 1 << 16, FAKE), ("NULL x", cap4, None, 2, 2,
                                       FAKE),
                                   ("NULL kg", cap4, FAKE, 2, 2, None)):
        add("plan_forward_batches " + label, lib.dkg_plan_forward_batches, ref(p), FAKE, x, B, nb, kg, None)
    add("plan_forward_grad NULL plan", lib.dkg_plan_forward_grad, None, FAKE, FAKE, 1, FAKE, FAKE, None)
    add("plan_forward_grad_hostx NULL plan", lib.dkg_plan_forward_grad_hostx, ref(grad4), None, FAKE, FAKE, 1, FAKE,
        FAKE,
        None, None)
    xh = (c_double * 128)()
    for label, p, x, B, g in (("no GRAD", cap4, FAKE, 1, FAKE), ("blank B=0: no GRAD first", blank, FAKE, 0, FAKE),
                              ("B=-1", grad4, FAKE, -1, FAKE), ("B=0", grad4, None, 0, None), ("B=5 of 4", grad4, FAKE,
                                  5, FAKE),
                              ("NULL x", grad4, None, 1, FAKE), ("NULL dkg_dx", grad4, FAKE, 1, None),
                              ("B=5 d=16", grad16, FAKE, 5, FAKE), ("B=9 of 8 d=16", grad16, FAKE, 9, FAKE)):
        if "d=16" not in label or "of" in label:
            add("plan_forward_grad " + label, lib.dkg_plan_forward_grad, ref(p), FAKE, x, B, FAKE, g, None)
        add("plan_forward_grad_hostx " + label, lib.dkg_plan_forward_grad_hostx, ref(p), FAKE, xh if x else None, FAKE,
            B,
            FAKE, g, None, None)
    add("plan_forward_grad_hostx NULL x_dev", lib.dkg_plan_forward_grad_hostx, ref(grad4), FAKE, xh, None, 1, FAKE,
        FAKE,
        None, None)
    err = c_int(0)
    add("plan_status NULL plan", lib.dkg_plan_status, None, ref(err), 0, None)
    add("plan_status NULL err", lib.dkg_plan_status, ref(cap4), None, 0, None)
    for label, p, o, B in (("NULL plan", None, FAKE, 1), ("NULL out", cap4, None, 1), ("B=-1", cap4, FAKE, -1),
                           ("B=5 of 4", cap4, FAKE, 5), ("B=0", cap4, FAKE, 0), ("two targets B=0", two, FAKE, 0)):
        add("plan_hull_sizes " + label, lib.dkg_plan_hull_sizes, ref(p) if p else None, o, B, None)
    avg = ctypes.c_float(0)
    for label, p, dev, x, B, kg, stage, reps, a in (
            ("NULL plan", None, FAKE, FAKE, 1, FAKE, 0, 1, avg), ("NULL device plan", cap4, None, FAKE, 1, FAKE, 0, 1,
                avg),
            ("NULL avg_ms", cap4, FAKE, FAKE, 1, FAKE, 0, 1, None), ("stage=4", cap4, FAKE, FAKE, 1, FAKE, 4, 1, avg),
            ("stage=-1", cap4, FAKE, FAKE, 1, FAKE, -1, 1, avg), ("reps=0", cap4, FAKE, FAKE, 1, FAKE, 0, 0, avg),
            ("B=0", cap4, FAKE, FAKE, 0, FAKE, 0, 1, avg), ("B=5 of 4", cap4, FAKE, FAKE, 5, FAKE, 0, 1, avg),
            ("NULL x", cap4, FAKE, None, 1, FAKE, 0, 1, avg), ("NULL kg", cap4, FAKE, FAKE, 1, None, 3, 2, avg)):
        add("plan_time_stage " + label, lib.dkg_plan_time_stage, ref(p) if p else None, dev, x, B, kg, None, None,
            stage,
            reps, ref(a) if a is not None else None)
    for label, p, dev, B, nb, stage in (("B=0", cap4, FAKE, 0, 1, 0), ("nbatch=0 NULL plan", None, FAKE, 1, 0, 0),
                                        ("NULL plan", None, FAKE, 1, 1, 0), ("two targets", two, FAKE, 1, 1, 0),
                                        ("3 x 2 of 4", cap4, FAKE, 2, 3, 0), ("2^16 x 2^16", cap4, FAKE, 1 << 16,
                                            1 << 16, 0),
                                        ("NULL device plan", cap4, None, 2, 2, 0), ("stage=4", cap4, FAKE, 2, 2, 4)):
        add("plan_time_stage_batches " + label, lib.dkg_plan_time_stage_batches, ref(p) if p else None, dev, FAKE, B,
            nb,
            FAKE, None, stage, 1, ref(avg))
    for label, p, dev, x, B, a in (("NULL plan", None, FAKE, FAKE, 1, FAKE), ("NULL device plan", cap4, None, FAKE, 1,
        FAKE),
                                   ("B=-1", cap4, FAKE, FAKE, -1, FAKE), ("B=5 of 4", cap4, FAKE, FAKE, 5, FAKE),
                                   ("B=0", cap4, FAKE, None, 0, None), ("NULL x", cap4, FAKE, None, 1, FAKE),
                                   ("NULL intercepts", cap4, FAKE, FAKE, 1, None),
                                   ("two targets, one double per candidate", two, FAKE, FAKE, 1, FAKE)):
        add("plan_lines " + label, lib.dkg_plan_lines, ref(p) if p else None, dev, x, B, a, FAKE, None)
    o4 = (c_int * 4)()
    add("debug_plan_envelope NULL plan", lib.dkg_debug_plan_envelope, None, o4)
    add("debug_plan_envelope NULL out", lib.dkg_debug_plan_envelope, ref(blank), None)
    for label, p, o, B, h in (("NULL plan", None, 0, 1, FAKE), ("NULL out", f32p, 0, 1, None), ("no F32", cap4, 0, 1,
        FAKE),
                              ("output=2 of 2", f32p, 2, 1, FAKE), ("output=-1", f32p, -1, 1, FAKE), ("B=0", f32p, 0,
                                  0, FAKE),
                              ("B=5 of 4", f32p, 1, 5, FAKE)):
        add("debug_plan_qx32 " + label, lib.dkg_debug_plan_qx32, ref(p) if p else None, o, B, h, None)

    # ---- state preparation: (o, d, y, max_tries, L, work, bytes, alpha, root, jitter, stream)
    def prepare(label, at=None, d=3, y=FAKE, tries=3, Lp=FAKE, work=FAKE, nbytes=0, alpha=FAKE, root=FAKE,
        null_o=False):
        o = None if null_o else ref(_outs((37,), at)[0])
        add("prepare_output " + label, lib.dkg_prepare_output, o, d, y, tries, Lp, work, nbytes, alpha, root, None,
            None)

    prepare("NULL output", null_o=True)
    for label, kw in (("NULL y", {"y": None}), ("NULL L", {"Lp": None}), ("NULL work", {"work": None}),
                      ("NULL alpha", {"alpha": None}), ("NULL root", {"root": None}), ("d=0", {"d": 0}), ("d=17",
                          {"d": 17}),
                      ("max_tries=-1", {"tries": -1}), ("short workspace", {}),
                      ("one byte short", {"nbytes": lib.dkg_prepare_workspace(37) - 1}),
                      ("max_tries=-1 with a short workspace", {"tries": -1, "nbytes": 1})):
        prepare(label, **kw)
    for label, fields in (("n=0", {"n": 0}), ("n=1025", {"n": 1025}), ("kernel id 4", {"kernel": 4}),
                          ("NULL lengthscale", {"inv_lengthscale": None}), ("NULL train_x", {"train_x": None}),
                          ("a NULL alpha in the output is not read", {"alpha": None}), ("n=0 d=17", {"n": 0})):
        prepare(label, at={0: fields}, d=17 if "d=17" in label else 3)

    def arr(vals, typ=c_void_p):
        return None if vals is None else (typ * len(vals))(*vals)

    def prepares(label, ns=(37, 36, 16), at=None, m=None, d=3, y=(FAKE,) * 3, tries=3, Lp=(FAKE,) * 3, work=(FAKE,) * 3,
                 nbytes=(0, 0, 0), alpha=(FAKE,) * 3, root=(FAKE,) * 3, null_outs=False):
        add("prepare_outputs " + label, lib.dkg_prepare_outputs, None if null_outs else _outs(ns, at),
            len(ns) if m is None else m, d, arr(y), tries, arr(Lp), arr(work), arr(nbytes, c_size_t), arr(alpha),
                arr(root),
            None, None)

    prepares("NULL outs", null_outs=True)
    for label, kw in (("m=0", {"m": 0}), ("m=9", {"m": 9}), ("NULL train_y", {"y": None}), ("NULL L", {"Lp": None}),
                      ("NULL work", {"work": None}), ("NULL work_bytes", {"nbytes": None}), ("NULL alpha",
                          {"alpha": None}),
                      ("NULL root_frag", {"root": None}), ("m=9 with NULL train_y", {"m": 9, "y": None}),
                      ("NULL train_y[1]", {"y": (FAKE, None, FAKE), "nbytes": (1 << 20, 0, 0)}),
                      ("NULL work[2]", {"work": (FAKE, FAKE, None), "nbytes": (1 << 20, 1 << 20, 0)}),
                      ("d=17", {"d": 17}), ("max_tries=-1", {"tries": -1}), ("short workspaces", {}),
                      ("output 2 alone short", {"nbytes": (1 << 20, 1 << 20, 2303)}),
                      ("output 1 n=0", {"at": {1: {"n": 0}}, "nbytes": (1 << 20, 0, 0)}),
                      ("output 0 n=0 before output 1 kernel id", {"at": {0: {"n": 0}, 1: {"kernel": 7}}}),
                      ("output 0 workspace before output 1 kernel id", {"at": {1: {"kernel": 7}}})):
        prepares(label, **kw)

    # ---- the MLL: (outs, m, d, train_y, max_tries, work, bytes, value, grad, jitter, stream)
    def mll(label, ns=(37, 36, 16), at=None, m=None, d=3, y=(FAKE,) * 3, tries=3, work=FAKE, nbytes=0, value=FAKE,
        grad=FAKE,
            null_outs=False):
        add("mll " + label, lib.dkg_mll_value_grad, None if null_outs else _outs(ns, at), len(ns) if m is None else m,
            d,
            arr(y), tries, work, nbytes, ctypes.cast(value, ctypes.POINTER(c_double)),
            ctypes.cast(grad, ctypes.POINTER(c_double)), None, None)

    mll("NULL outs", null_outs=True)
    for label, kw in (("NULL train_y", {"y": None}), ("NULL work", {"work": None}), ("NULL value", {"value": None}),
                      ("NULL grad", {"grad": None}), ("m=0", {"m": 0}), ("m=9", {"m": 9}), ("d=0", {"d": 0}), ("d=17",
                          {"d": 17}),
                      ("m=9 d=17", {"m": 9, "d": 17}), ("m=0 d=17", {"m": 0, "d": 17}), ("max_tries=-1", {"tries": -1}),
                      ("d=17 max_tries=-1", {"d": 17, "tries": -1}), ("NULL train_y[1]", {"y": (FAKE, None, FAKE)}),
                      ("NULL train_y[1] behind a valid output 0, output 2 n=0", {"y": (FAKE, None, FAKE),
                          "at": {2: {"n": 0}}}),
                      ("output 0 n=0 before NULL train_y[1]", {"y": (FAKE, None, FAKE), "at": {0: {"n": 0}}}),
                      ("output 1 n=0", {"at": {1: {"n": 0}}}), ("output 1 n=1025", {"at": {1: {"n": 1025}}}),
                      ("output 1 n=1009 is fine", {"at": {1: {"n": 1009}}}), ("output 2 kernel id",
                          {"at": {2: {"kernel": 4}}}),
                      ("output 1 NULL lengthscale", {"at": {1: {"inv_lengthscale": None}}}),
                      ("output 1 NULL train_x", {"at": {1: {"train_x": None}}}),
                      ("a NULL alpha is not read", {"at": {1: {"alpha": None, "root_frag": None}}}),
                          ("short workspace", {}),
                      ("one byte short", {"nbytes": lib.dkg_mll_workspace((c_int * 3)(37, 36, 16), 3) - 1}),
                      ("m=1", {"ns": (1024,), "y": (FAKE,)})):
        mll(label, **kw)

    # ---- kernel matrix, roots: (o, d, x1, n1, x2, n2, diag, out, stream)
    one = _outs((37,))
    for label, o, d, x1, n1, x2, n2, res in (
            ("NULL output", None, 3, FAKE, 5, FAKE, 5, FAKE), ("NULL x1", one, 3, None, 5, FAKE, 5, FAKE),
            ("NULL x2", one, 3, FAKE, 5, None, 5, FAKE), ("NULL out", one, 3, FAKE, 5, FAKE, 5, None),
            ("NULL lengthscale", _outs((37,), {0: {"inv_lengthscale": None}}), 3, FAKE, 5, FAKE, 5, FAKE),
            ("d=0", one, 0, FAKE, 5, FAKE, 5, FAKE), ("d=17", one, 17, FAKE, 5, FAKE, 5, FAKE),
            ("d=17 n1=-1", one, 17, FAKE, -1, FAKE, 5, FAKE), ("n1=-1", one, 3, FAKE, -1, FAKE, 5, FAKE),
            ("n2=-1 n1=0", one, 3, FAKE, 0, FAKE, -1, FAKE), ("n1=0", one, 3, FAKE, 0, FAKE, 5, FAKE),
            ("n2=0", one, 3, FAKE, 5, FAKE, 0, FAKE)):
        add("kernel_matrix " + label, lib.dkg_kernel_matrix, o, d, x1, n1, x2, n2, 0.0, res, None)
    add("pack_root NULL r", lib.dkg_pack_root, None, 5, FAKE, None)
    add("pack_root NULL root_frag", lib.dkg_pack_root, FAKE, 5, None, None)
    add("pack_root n=0", lib.dkg_pack_root, FAKE, 0, FAKE, None)
    for label, o, d, x, r, q in (("NULL output", None, 3, FAKE, 5, FAKE), ("d=17", one, 17, FAKE, 5, FAKE),
                                 ("n=0", _outs((0,)), 3, FAKE, 5, FAKE), ("NULL root", _outs((37,),
                                     {0: {"root_frag": None}}), 3, FAKE, 5, FAKE),
                                 ("rows=-1", one, 3, FAKE, -1, FAKE), ("NULL q_frag", one, 3, FAKE, 5, None),
                                 ("NULL x", one, 3, None, 5, FAKE), ("rows=0", one, 3, None, 0, FAKE),
                                 ("rows=0 NULL q_frag", one, 3, None, 0, None), ("rows=0 d=17", one, 17, None, 0,
                                     FAKE)):
        add("cross_root " + label, lib.dkg_cross_root, o, d, x, r, q, None, None)

    # ---- append: (o, d, L, Linv, disc, N, x, y, jitter, L', Linv', alpha', root', disc_frag', disc_mean', work,
    # bytes, stream)
    def append(label, n=37, at=None, d=3, L_=FAKE, disc=FAKE, N=50, x=FAKE, jitter=0.0, Ln=FAKE, qn=FAKE, mn=FAKE,
        work=FAKE,
               nbytes=0, null_o=False):
        o = None if null_o else ref(_outs((n,), at)[0])
        add("append " + label, lib.dkg_append_observation, o, d, L_, FAKE, disc, N, x, FAKE, jitter, Ln, FAKE, FAKE,
            FAKE, qn,
            mn, work, nbytes, None)

    append("NULL output", null_o=True)
    for label, kw in (("NULL L", {"L_": None}), ("NULL train_x", {"x": None}), ("NULL L_new", {"Ln": None}),
                      ("NULL work", {"work": None}), ("NULL lengthscale", {"at": {0: {"inv_lengthscale": None}}}),
                      ("N=-1", {"N": -1}), ("N=-1 with n=1024", {"N": -1, "n": 1024}), ("NULL disc", {"disc": None}),
                      ("NULL disc at N=0 is fine", {"disc": None, "N": 0, "qn": None, "mn": None}),
                      ("NULL disc_frag", {"at": {0: {"disc_frag": None}}}), ("NULL disc_frag_new", {"qn": None}),
                      ("NULL disc_mean_new", {"mn": None}), ("n=0", {"n": 0}), ("n=1024", {"n": 1024}),
                      ("n=1023 is fine", {"n": 1023}), ("d=0", {"d": 0}),
                      ("d=17", {"d": 17}), ("n=1024 d=17", {"n": 1024, "d": 17}), ("N=2^22+1", {"N": (1 << 22) + 1}),
                      ("kernel id", {"at": {0: {"kernel": 4}}}), ("jitter=-1", {"jitter": -1.0}),
                      ("jitter=nan", {"jitter": float("nan")}), ("jitter=-1 kernel id", {"jitter": -1.0,
                          "at": {0: {"kernel": 4}}}),
                      ("short workspace", {}), ("one byte short", {"nbytes": lib.dkg_append_workspace(37, 50) - 1})):
        append(label, **kw)

    # ---- lines: (a, b, P, L, kg, n_hull, stream); (a, b, P, L, cap, idx, xs, count, stream);
    # (a, b, c, P, m, out, stream)
    for label, a, b, P, L_, kg in (("P=-1", FAKE, FAKE, -1, 3, FAKE), ("L=-1", FAKE, FAKE, 3, -1, FAKE),
                                   ("P=0", None, None, 0, 0, None), ("L=0", FAKE, FAKE, 3, 0, FAKE),
                                   ("NULL intercepts", None, FAKE, 3, 3, FAKE), ("NULL slopes", FAKE, None, 3, 3, FAKE),
                                   ("NULL kg", FAKE, FAKE, 3, 3, None), ("L=0 NULL kg", FAKE, FAKE, 3, 0, None)):
        add("lines_kg " + label, lib.dkg_lines_kg, a, b, P, L_, kg, None, None)
    for label, a, P, L_, cap, idx, xs, cnt in (("P=-1", FAKE, -1, 3, 4, FAKE, FAKE, FAKE), ("cap=0", FAKE, 3, 3, 0,
        FAKE, FAKE, FAKE),
                                               ("P=0", None, 0, 3, 4, None, None, None), ("L=0", FAKE, 3, 0, 4, FAKE,
                                                   FAKE, FAKE),
                                               ("NULL intercepts", None, 3, 3, 4, FAKE, FAKE, FAKE),
                                               ("NULL indices", FAKE, 3, 3, 4, None, FAKE, FAKE),
                                               ("NULL count", FAKE, 3, 3, 4, FAKE, FAKE, None),
                                               ("NULL intersections at cap=4", FAKE, 3, 3, 4, FAKE, None, FAKE)):
        add("epigraph " + label, lib.dkg_epigraph, a, FAKE, P, L_, cap, idx, xs, cnt, None)
    for label, a, c, P, m, res in (("P=-1", FAKE, FAKE, -1, 3, FAKE), ("m=-1", FAKE, FAKE, 3, -1, FAKE), ("P=0", None,
        None, 0, 3, None),
                                   ("m=0", FAKE, FAKE, 3, 0, FAKE), ("NULL intercepts", None, FAKE, 3, 3, FAKE),
                                   ("NULL out", FAKE, FAKE, 3, 3, None), ("NULL boundaries at m=2", FAKE, None, 3, 2,
                                       FAKE)):
        add("pwl_expectation " + label, lib.dkg_pwl_expectation, a, FAKE, c, P, m, res, None)

    # ---- debug entries
    add("debug_read_kstamps NULL host", lib.dkg_debug_read_kstamps, None, 8)
    add("debug_read_kstamps n=-1", lib.dkg_debug_read_kstamps, FAKE, -1)
    add("debug_read_kstamps without stamps", lib.dkg_debug_read_kstamps, ctypes.create_string_buffer(64), 8)
    add("debug_cross_tall mode=2", lib.dkg_debug_cross_tall, 2)
    add("debug_cross_tall mode=-2", lib.dkg_debug_cross_tall, -2)
    for a in ((24, 3, 1, 0), (16, 17, 1, 0), (16, 3, 0, 1)):
        add(f"debug_cross_tall_eligible {a}", lib.dkg_debug_cross_tall_eligible, *a)
    o6 = (c_int * 6)()
    for label, a, o in (("NULL out", (256, 3, 50, 2, 17, 0), None), ("max_n_pad=1040", (1040, 3, 50, 2, 17, 0), o6),
                        ("m=9", (256, 3, 50, 9, 17, 0), o6), ("geom_B=-1", (256, 3, 50, 2, 17, -1), o6)):
        add("debug_f32_dispatch " + label, lib.dkg_debug_f32_dispatch, *a, o)
    o21 = (c_int * (ENV_REGIONS + 1))()
    for label, a, o in (("NULL out", ENV_LDS[1], None), ("m=9", (9, 50, 8, 8, 3, 256, 0, 0, 0), o21),
                        ("N=2^22+1", (2, (1 << 22) + 1, 8, 8, 3, 256, 0, 0, 0), o21), ("waves=9", (2, 50, 9, 8, 3, 256,
                            0, 0, 0), o21),
                        ("S x m > 2^24", (8, 50, 8, (1 << 21) + 1, 3, 256, 0, 0, 0), o21), ("max_np=24", (2, 50, 8, 8,
                            3, 24, 0, 0, 0), o21),
                        ("grows without grad", (2, 50, 8, 8, 3, 256, 0, 1, 1), o21),
                        ("grows without stream", (2, 50, 8, 8, 3, 256, 1, 0, 1), o21),
                        ("m=9 and grows without grad", (9, 50, 8, 8, 3, 256, 0, 0, 1), o21)):
        add("debug_envelope_lds " + label, lib.dkg_debug_envelope_lds, *a, o)
    add("debug_wave_ops NULL in", lib.dkg_debug_wave_ops, None, FAKE, None)
    add("debug_wave_ops NULL out", lib.dkg_debug_wave_ops, FAKE, None, None)
    add("debug_mfma_f64 NULL a", lib.dkg_debug_mfma_f64, None, FAKE, FAKE, None)
    add("debug_mfma_f64 NULL c", lib.dkg_debug_mfma_f64, FAKE, FAKE, None, None)

    # ---- the launcher (csrc/dkg_launch.hip); one thread: the caller alone, no worker is started
    add("launcher_create NULL handle", lib.dkg_launcher_create, 1, None)
    add("launcher_create threads=0", lib.dkg_launcher_create, 0, ref(c_void_p()))
    add("launcher_create threads=65", lib.dkg_launcher_create, 65, ref(c_void_p()))
    add("launcher_arm NULL", lib.dkg_launcher_arm, None, 0.0)
    add("launcher_graphs NULL", lib.dkg_launcher_graphs, None, 0, None, None, None)
    add("launcher_destroy NULL", lib.dkg_launcher_destroy, None)
    handle = c_void_p()
    add("launcher_create", lib.dkg_launcher_create, 1, ref(handle))
    one_ptr, down = (c_void_p * 1)(FAKE), (c_int * 2)(1, 0)
    add("launcher_graphs n_streams=-1", lambda: lib.dkg_launcher_graphs(handle, -1, one_ptr, down, one_ptr))
    add("launcher_graphs NULL streams", lambda: lib.dkg_launcher_graphs(handle, 1, None, down, one_ptr))
    add("launcher_graphs NULL offsets", lambda: lib.dkg_launcher_graphs(handle, 1, one_ptr, None, one_ptr))
    add("launcher_graphs NULL graphs", lambda: lib.dkg_launcher_graphs(handle, 1, one_ptr, down, None))
    add("launcher_graphs offsets going down", lambda: lib.dkg_launcher_graphs(handle, 1, one_ptr, down, one_ptr))
    add("launcher_graphs no streams", lambda: lib.dkg_launcher_graphs(handle, 0, None, None, None))
    add("launcher_destroy", lambda: lib.dkg_launcher_destroy(handle))
    return out


def record():
    """What the fixture holds, from the library that is loaded."""
    assert "DKG_DEBUG_STAMPS" not in os.environ and "DKG_ENV_SW" not in os.environ
    lib = _lib().load()
    values = {name: [t() for t in thunks] for name, thunks in queries().items()}
    replayed = []
    for label, thunk in calls():
        status = int(thunk())
        replayed.append([status, lib.dkg_last_error().decode() if status else ""])
    return {"queries": values, "calls": replayed}


def _golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_host.json")) as f:
        return json.load(f)


def test_the_grids_turn_every_section_on_and_off():
    """Every value of every axis survives the thinning, and so does each pairing that a condition reads."""
    def seen(grid, *cols):
        return {tuple(row[c] for c in cols) for row in grid}

    assert 100 <= len(FORWARD_GRID) and 100 <= len(PLAN_GRID) and 100 <= len(TARGETS_GRID)
    assert len(FORWARD_GRID) + len(PLAN_GRID) + len(TARGETS_GRID) <= 600
    for grid, axes in ((FORWARD_GRID, (NS, _N, _B, _S)), (PLAN_GRID, (NS, _D, _N, _B, _S, _FLAGS))):
        for c, axis in enumerate(axes):
            assert seen(grid, c) == {(v,) for v in axis}
    assert seen(PLAN_GRID, 5, 1) == set(itertools.product(_FLAGS, _D))  # GRAD with d
    assert {(f, _fill(ns, B)) for ns, d, N, B, S, f in PLAN_GRID} == set(itertools.product(_FLAGS, (False, True)))
    assert {(f, N + 1 <= 64 * 33) for ns, d, N, B, S, f in PLAN_GRID} == set(itertools.product(_FLAGS, (False, True)))
    assert seen(PLAN_GRID, 5, 4) == set(itertools.product(_FLAGS, _S))  # GRAD with the split (wg_gpart)
    kinds = {(0 if T == 1 else 1 if T == 2 else 2) for ns, d, N, B, S, T, f in TARGETS_GRID if len(ns) > 1}
    assert kinds == {0, 1, 2} and seen(TARGETS_GRID, 6) == {(f,) for f in _FLAGS}
    multi = [row for row in TARGETS_GRID if row[5] > 1]
    assert seen(multi, 3) == {(v,) for v in _B} and seen(multi, 4) == {(v,) for v in _S}  # T with B and S
    assert seen(multi, 2) == {(v,) for v in _N} and seen(multi, 1) == {(v,) for v in _D}
    assert {len(row[0]) for row in multi} == {1, 2, 3, 8}


def test_queries_are_the_recorded_ones():
    want, got = _golden()["queries"], record()["queries"]
    assert sorted(want) == sorted(got)
    for name in got:
        assert len(got[name]) == len(want[name]), name
        for i, (g, w) in enumerate(zip(got[name], want[name])):
            assert g == w, (name, i, g, w)
    for name in ("dkg_forward_workspace", "dkg_plan_workspace", "dkg_plan_workspace_targets", "dkg_prepare_workspace",
                 "dkg_mll_workspace", "dkg_append_workspace"):
        assert 0 in want[name] and max(want[name]) > 0
    assert set(want["dkg_plan_grad_rows"]) == {0, 1, -1, -2}
    assert all(row[0] == 0 for row in want["dkg_debug_envelope_lds"])


def test_calls_are_the_recorded_ones():
    L = _lib()
    labels = [label for label, _ in calls()]
    want, got = _golden()["calls"], record()["calls"]
    assert len(want) == len(got) == len(labels)
    for label, w, g in zip(labels, want, got):
        # no device was there when the fixture was recorded: a HIP status or a failed factorisation cannot be in it
        assert w[0] in (L.DKG_OK, L.DKG_ERR_ARG, L.DKG_ERR_UNSUPPORTED, L.DKG_ERR_WORKSPACE, L.DKG_ERR_NO_LINES, -1,
            -2), label
        assert g == w, (label, w, g)
    text = " | ".join(w[1] for w in want)
    for pinned in ("negative size B=-1 N=50", "negative size N=-1", "m=9 outputs (supported 1..8)",
        "m=9 outputs (1..8)",
                   "output 0: n=0 training points", "unknown plan flags 0x41",
                       "weights exceed the envelope stage's LDS",
                   "targets[1]=1 repeats targets[0]", "T=5 targets (1..4 for 3 outputs)",
                       "DKG_PLAN_FUSED runs one target",
                   "N=-1 discretisation points", "graph offsets not increasing at stream 0",
                       "launcher threads=65 (1..64)",
                   "exceed the cross stage's LDS budget",
                       "gradient: m=2 outputs, n=800, d=6 exceed the envelope stage's LDS"):
        assert pinned in text, pinned
    assert sum(w[0] == L.DKG_OK for w in want) >= 20
