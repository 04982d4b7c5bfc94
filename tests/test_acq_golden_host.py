"""The workspace sizes and the refusals of the acquisition layer's C entries (dkg_pareto, dkg_jes, dkg_rff, dkg_hvkg,
dkg_boxes), pinned to a recording (no GPU: a size query launches nothing, and an argument check returns before any
launch, as the other ``*_host`` tests rely on).

``tests/golden/acq_host.json`` holds, for every ``dkg_*_workspace`` query, the value at each argument tuple of
``QUERIES`` (the limits, one past each limit, which gives 0, and ragged sizes), and for every call of ``refusals()``
its ``(status, dkg_last_error())``.  It was recorded from the build of the commit before the one that moved these
entries' carves and checks into csrc/dkg_acq.h, with that build's library in ``DKG_LIB``, from the repository root:

    import json, sys
    sys.path[:0] = ["tests", "decoupled-kg_amd"]
    import test_acq_golden_host as t
    json.dump(t.record(), open("tests/golden/acq_host.json", "w"), indent=1)

The test replays both lists and compares for equality: a byte of a message, a status or a byte of a workspace that
moves fails it.
"""

import ctypes
import json
import os

S, K, M = 3, 70, 3
_P = (8, 1024)
_R = (1, 70, 1024)
_B = (1, 17, 4096)
_D = (1, 3, 16)

# entry -> argument tuples
QUERIES = {
    "dkg_pareto_rank_workspace": [(Q, m) for Q in (1, 37, K, 2048, 2049, 16384) for m in (1, M, 8)]
                                 + [(0, M), (16385, M), (K, 0), (K, 9)],
    "dkg_pareto_workspace": [(P, d, M) for P in _P for d in _D]
                            + [(12, 5, 8), (4, 3, M), (10, 3, M), (1028, 3, M), (8, 0, M), (8, 17, M), (8, 3, 0), (8, 3, 9)],
    "dkg_pareto_paths_workspace": [(s, P, d, M) for s in (1, S, 64) for P in _P for d in (1, 16)]
                                  + [(0, 8, 3, M), (65, 8, 3, M), (S, 1028, 3, M), (S, 8, 17, M), (S, 8, 3, 9)],
    "dkg_rff_workspace": [(R, n) for R in _R for n in (1, 37, 100, 1024)]
                         + [(0, 37), (1025, 37), (K, 0), (K, 1025)],
    "dkg_jes_workspace": [(M, P, d, K, B) for P in (1, 2, 64) for d in _D for B in (1, 17, 4096, 65536)]
                         + [(8, 64, 16, 4096, 17), (9, 2, 3, K, 17), (M, 65, 3, K, 17), (M, 2, 17, K, 17),
                            (M, 2, 3, 4097, 17), (M, 2, 3, K, 65537), (0, 2, 3, K, 17), (M, 2, 3, 0, 17)],
    "dkg_hvkg_workspace": [(m, d, Nf, Np, B) for m in (2, 3) for d in _D for (Nf, Np) in ((1, 1), (3, 4), (64, 32))
                           for B in _B]
                          + [(1, 3, 3, 4, 17), (4, 3, 3, 4, 17), (M, 17, 3, 4, 17), (M, 3, 65, 4, 17), (M, 3, 3, 33, 17),
                             (M, 3, 3, 4, 4097), (M, 0, 3, 4, 17)],
    "dkg_dominated_boxes_workspace": [(s, k, m) for s in (1, S, 65535) for k in (1, K, 2048) for m in (1, 2, 3)]
                                     + [(0, K, M), (65536, K, M), (S, 2049, M), (S, K, 4), (S, K, 0)],
    "dkg_hypervolume_front_workspace": [(s, k, m) for s in (1, S, 65535) for k in (1, K, 16384) for m in (1, 2, 3)]
                                       + [(0, K, M), (65536, K, M), (S, 16385, M), (S, K, 4), (S, 0, M)],
}

FAKE = 64  # a pointer that is never followed: the checks come first


def _lib():
    from dkg_amd import _lib as L

    return L


def _outputs(count, n=5, **bad):
    """`count` outputs of fake pointers; bad: {index: {field: value}}."""
    outs = (_lib().DkgOutput * count)()
    for o in outs:
        o.n, o.kernel, o.outputscale, o.noise, o.y_std = n, 2, 1.0, 1e-2, 1.0
        o.inv_lengthscale = o.train_x = o.alpha = o.root_frag = FAKE
    for i, fields in bad.get("at", {}).items():
        for k, v in fields.items():
            setattr(outs[i], k, v)
    return outs


def _paths(S_=S, m=M, d=3, R=K, omega=FAKE):
    return _lib().DkgRffPaths(S_, m, d, R, omega, FAKE, FAKE, FAKE)


def refusals():
    """[(label, thunk)]: every thunk is a call that is refused before any device work."""
    L = _lib()
    lib = L.load()
    ref = (ctypes.c_double * 4)(0.0, 0.0, 0.0, 0.0)
    z = (ctypes.c_double * (65 * 4))()
    prm = L.DkgNsga2Params(0.95, 10.0, 0.01, 50.0)
    big = 1 << 40
    calls = []

    def add(label, fn, *args):
        calls.append((label, lambda: fn(*args)))

    # ---- joint entropy search: (states, m, P, d, bounds, J, target, only_diagonal, max_B, ws, bytes, plan, stream)
    jes_host = ctypes.create_string_buffer(lib.dkg_jes_plan_bytes())

    def jes(label, states=None, m=2, P=2, d=3, bounds=FAKE, J=K, target=-1, max_B=17, ws=FAKE, nbytes=big, host=jes_host,
            null_states=False):
        st = None if null_states else (states if states is not None else _outputs(32))
        add("jes_init " + label, lib.dkg_jes_init, st, m, P, d, bounds, J, target, 0, max_B, ws, nbytes, host, None)

    jes("NULL states", null_states=True)
    jes("NULL bounds", bounds=None)
    jes("NULL workspace", ws=None)
    jes("NULL plan", host=None)
    for label, kw in (("m=0", {"m": 0}), ("m=9", {"m": 9}), ("d=0", {"d": 0}), ("d=17", {"d": 17}), ("P=0", {"P": 0}),
                      ("P=65", {"P": 65}), ("J=0", {"J": 0}), ("J=4097", {"J": 4097}), ("max_B=0", {"max_B": 0}),
                      ("max_B=65537", {"max_B": 65537}), ("target=m", {"target": 2}), ("target=-2", {"target": -2}),
                      ("m=9 d=17", {"m": 9, "d": 17}), ("short workspace", {"nbytes": 255})):
        jes(label, **kw)
    for label, fields in (("kernel id", {"kernel": 7}), ("n=0", {"n": 0}), ("n=1025", {"n": 1025}),
                          ("NULL alpha", {"alpha": None}), ("NULL root", {"root_frag": None}),
                          ("NULL train_x", {"train_x": None}), ("NULL lengthscale", {"inv_lengthscale": None})):
        jes("state 2 output 1 " + label, states=_outputs(6, at={5: fields}))
    jes("state 0 output 0 n=0 before state 2 output 1", states=_outputs(6, at={0: {"n": 0}, 5: {"kernel": 7}}))
    blank = ctypes.create_string_buffer(lib.dkg_jes_plan_bytes())
    add("jes_forward NULL plan", lib.dkg_jes_forward, None, FAKE, 1, FAKE, None, None, None)
    add("jes_forward NULL x", lib.dkg_jes_forward, blank, None, 1, FAKE, None, None, None)
    add("jes_forward NULL acq", lib.dkg_jes_forward, blank, FAKE, 1, None, None, None, None)
    add("jes_forward uninitialised", lib.dkg_jes_forward, blank, FAKE, 1, FAKE, None, None, None)

    # ---- HVKG: (outs, m, d, ref, Nf, Np, z, mask, current, cost, max_B, ws, bytes, plan, stream)
    hv_host = ctypes.create_string_buffer(lib.dkg_hvkg_plan_bytes())

    def hvkg(label, outs=None, m=2, d=3, ref_=ref, Nf=3, Np=4, z_=z, mask=1, cur=0.0, cost=1.0, max_B=17, ws=FAKE,
             nbytes=big, host=hv_host, null_outs=False):
        o = None if null_outs else (outs if outs is not None else _outputs(4))
        add("hvkg_init " + label, lib.dkg_hvkg_init, o, m, d, ref_, Nf, Np, z_, mask, cur, cost, max_B, ws, nbytes, host,
            None)

    hvkg("NULL outs", null_outs=True)
    hvkg("NULL ref", ref_=None)
    hvkg("NULL base samples", z_=None)
    hvkg("NULL workspace", ws=None)
    hvkg("NULL plan", host=None)
    for label, kw in (("m=0", {"m": 0}), ("m=1", {"m": 1}), ("m=4", {"m": 4}), ("d=0", {"d": 0}), ("d=17", {"d": 17}),
                      ("Nf=0", {"Nf": 0}), ("Nf=65", {"Nf": 65}), ("Np=0", {"Np": 0}), ("Np=33", {"Np": 33}),
                      ("max_B=0", {"max_B": 0}), ("max_B=4097", {"max_B": 4097}), ("mask=4", {"mask": 4}),
                      ("empty mask Nf=3", {"mask": 0}), ("cost=0", {"cost": 0.0}), ("current=inf", {"cur": float("inf")}),
                      ("m=4 d=17", {"m": 4, "d": 17}), ("short workspace", {"nbytes": 255})):
        hvkg(label, **kw)
    for label, fields in (("kernel id", {"kernel": -1}), ("n=0", {"n": 0}), ("n=1025", {"n": 1025}),
                          ("NULL alpha", {"alpha": None}), ("NULL root", {"root_frag": None})):
        hvkg("output 1 " + label, outs=_outputs(2, at={1: fields}))
    hblank = ctypes.create_string_buffer(lib.dkg_hvkg_plan_bytes())
    add("hvkg_forward NULL plan", lib.dkg_hvkg_forward, None, FAKE, 1, FAKE, None, None, None)
    add("hvkg_forward NULL x", lib.dkg_hvkg_forward, hblank, None, 1, FAKE, None, None, None)
    add("hvkg_forward uninitialised", lib.dkg_hvkg_forward, hblank, FAKE, 1, FAKE, None, None, None)
    for label, args in (("NULL Y", (None, 1, 4, 2, ref, FAKE)), ("NULL ref", (FAKE, 1, 4, 2, None, FAKE)),
                        ("NULL hv", (FAKE, 1, 4, 2, ref, None)), ("S=0", (FAKE, 0, 4, 2, ref, FAKE)),
                        ("Np=0", (FAKE, 1, 0, 2, ref, FAKE)), ("m=0", (FAKE, 1, 4, 0, ref, FAKE)),
                        ("m=1", (FAKE, 1, 4, 1, ref, FAKE)), ("m=4", (FAKE, 1, 4, 4, ref, FAKE)),
                        ("Np=33", (FAKE, 1, 33, 2, ref, FAKE))):
        add("hypervolume " + label, lib.dkg_hypervolume, *args, None, None)

    # ---- the posterior mean and the Pareto entries
    def mean(label, outs, m=M, d=3, x=FAKE, P=19, out=FAKE):
        add("posterior_mean " + label, lib.dkg_posterior_mean, outs, m, d, x, P, out, None)

    mean("NULL outs", None)
    for label, kw in (("m=0", {"m": 0}), ("m=9", {"m": 9}), ("d=0", {"d": 0}), ("d=17", {"d": 17}),
                      ("m=9 d=0", {"m": 9, "d": 0}), ("m=0 d=17", {"m": 0, "d": 17}), ("P=-1", {"P": -1}),
                      ("P=2^24+1", {"P": (1 << 24) + 1}), ("NULL x", {"x": None}), ("NULL mean", {"out": None})):
        mean(label, _outputs(9), **kw)
    for label, fields in (("kernel id", {"kernel": 9}), ("n=0", {"n": 0}), ("n=1025", {"n": 1025}),
                          ("NULL alpha", {"alpha": None}), ("NULL train_x", {"train_x": None})):
        mean("output 2 " + label, _outputs(M, at={2: fields}))
    mean("a NULL root is not read", _outputs(M, at={0: {"root_frag": None}, 1: {"n": 0}}))

    def rank(label, F=FAKE, Q=K, m=M, keep=1, out=FAKE, work=None, nbytes=0):
        add("pareto_rank " + label, lib.dkg_pareto_rank, F, Q, m, keep, out, out, out, work, nbytes, None)

    rank("Q=0", Q=0)
    rank("m=0", m=0)
    rank("keep=0", keep=0)
    rank("keep>Q", keep=K + 1)
    rank("Q=2049 without a workspace", Q=2049)
    rank("Q=16385 with a workspace", Q=16385, work=FAKE, nbytes=big)
    rank("m=9", m=9)
    rank("NULL F", F=None)
    rank("NULL outputs", out=None)
    rank("short workspace", work=FAKE, nbytes=255)

    def variation(label, X=FAKE, P=8, d=3, lb=FAKE, p=prm, out=FAKE):
        add("pareto_variation " + label, lib.dkg_pareto_variation, X, FAKE, FAKE, P, d, lb, FAKE, p, FAKE, out, None)

    for label, kw in (("P=6", {"P": 6}), ("P=10", {"P": 10}), ("P=1028", {"P": 1028}), ("d=0", {"d": 0}),
                      ("d=17", {"d": 17}), ("NULL params", {"p": None}),
                      ("cr=1.5", {"p": L.DkgNsga2Params(1.5, 10.0, 0.01, 50.0)}),
                      ("eta_m=-1", {"p": L.DkgNsga2Params(0.9, 10.0, 0.01, -1.0)}), ("NULL X", {"X": None}),
                      ("NULL lb", {"lb": None}), ("NULL children", {"out": None})):
        variation(label, **kw)

    def nsga2(label, outs, m=M, d=3, lb=FAKE, P=8, gens=2, p=prm, u=FAKE, X=FAKE, work=FAKE, nbytes=big):
        add("pareto_nsga2 " + label, lib.dkg_pareto_nsga2, outs, m, d, lb, FAKE, P, gens, p, u, X, FAKE, FAKE, FAKE, work,
            nbytes, None)

    nsga2("NULL outs", None)
    for label, kw in (("m=9", {"m": 9}), ("d=17", {"d": 17}), ("P=10", {"P": 10}), ("P=1028", {"P": 1028}),
                      ("gens=-1", {"gens": -1}), ("NULL params", {"p": None}), ("NULL lb", {"lb": None}),
                      ("NULL uniforms", {"u": None}), ("NULL X", {"X": None}), ("NULL workspace", {"work": None}),
                      ("short workspace", {"nbytes": 255})):
        nsga2(label, _outputs(9), **kw)
    nsga2("output 1 n=1025", _outputs(M, at={1: {"n": 1025}}))

    def paths_nsga2(label, paths, lb=FAKE, P=8, gens=2, p=prm, nbytes=big):
        add("pareto_nsga2_paths " + label, lib.dkg_pareto_nsga2_paths, paths, lb, FAKE, P, gens, p, FAKE, FAKE, FAKE, FAKE,
            FAKE, FAKE, nbytes, None)

    paths_nsga2("NULL paths", None)
    for label, kw in (("S=0", {"S_": 0}), ("S=65", {"S_": 65}), ("m=0", {"m": 0}), ("m=9", {"m": 9}), ("d=17", {"d": 17}),
                      ("m=9 d=17", {"m": 9, "d": 17}), ("R=0", {"R": 0}), ("R=1025", {"R": 1025}),
                      ("NULL omega", {"omega": None})):
        paths_nsga2(label, _paths(**kw))
    paths_nsga2("P=12 is fine, P=14 is not", _paths(), P=14)
    paths_nsga2("NULL lb", _paths(), lb=None)
    paths_nsga2("short workspace", _paths(), nbytes=255)

    def prune(label, F=FAKE, S_=S, Q=K, m=M, k=8, out=FAKE):
        add("pareto_prune " + label, lib.dkg_pareto_prune, F, FAKE, S_, Q, m, k, out, out, None)

    for label, kw in (("S=0", {"S_": 0}), ("k=0", {"k": 0}), ("S=65", {"S_": 65}), ("Q=2049", {"Q": 2049}),
                      ("k=2049", {"k": 2049}), ("m=9", {"m": 9}), ("NULL F", {"F": None}), ("NULL count", {"out": None})):
        prune(label, **kw)

    # ---- the sample paths
    add("rff_eval NULL paths", lib.dkg_rff_eval, None, FAKE, 19, 0, FAKE, None)
    add("rff_eval m=9", lib.dkg_rff_eval, _paths(m=9), FAKE, 19, 0, FAKE, None)
    add("rff_eval d=17", lib.dkg_rff_eval, _paths(d=17), FAKE, 19, 0, FAKE, None)
    add("rff_eval P=-1", lib.dkg_rff_eval, _paths(), FAKE, -1, 0, FAKE, None)
    add("rff_eval NULL x", lib.dkg_rff_eval, _paths(), None, 19, 0, FAKE, None)
    add("rff_eval NULL F", lib.dkg_rff_eval, _paths(), FAKE, 19, 0, None, None)
    ys = (ctypes.c_void_p * M)(FAKE, FAKE, FAKE)

    def weights(label, outs, m=M, d=3, y=ys, wn=FAKE, g=FAKE, tries=3, paths=None, work=FAKE, nbytes=big):
        add("rff_weights " + label, lib.dkg_rff_weights, outs, m, d, y, wn, g, FAKE, FAKE, tries,
            paths if paths is not None else _paths(), work, nbytes, None, None)

    weights("NULL outs", None)
    weights("R=1025", _outputs(M), paths=_paths(R=1025))
    weights("NULL train_y", _outputs(M), y=None)
    weights("NULL wn", _outputs(M), wn=None)
    weights("NULL workspace", _outputs(M), work=None)
    weights("m against the paths", _outputs(M), m=2)
    weights("d against the paths", _outputs(M), d=4)
    weights("max_tries=-1", _outputs(M), tries=-1)
    for label, fields in (("kernel id", {"kernel": 9}), ("n=0", {"n": 0}), ("n=1025", {"n": 1025}),
                          ("NULL train_x", {"train_x": None}), ("noise=0", {"noise": 0.0}),
                          ("outputscale=0", {"outputscale": 0.0})):
        weights("output 1 " + label, _outputs(M, at={1: fields}))
    weights("a NULL alpha is not read; NULL Gamma draws", _outputs(M, at={0: {"alpha": None}}), g=None)
    weights("short workspace", _outputs(M), nbytes=255)

    # ---- the boxes
    def boxes(label, Y=FAKE, S_=S, K_=K, m=M, ref_=ref, J=2 * K - 1, out=FAKE, work=FAKE, nbytes=big):
        add("dominated_boxes " + label, lib.dkg_dominated_boxes, Y, S_, K_, m, ref_, J, out, out, work, nbytes, None)

    def front(label, Y=FAKE, S_=S, K_=K, m=M, ref_=ref, out=FAKE, work=FAKE, nbytes=big):
        add("hypervolume_front " + label, lib.dkg_hypervolume_front, Y, S_, K_, m, ref_, out, work, nbytes, None)

    for fn in (boxes, front):
        for label, kw in (("NULL Y", {"Y": None}), ("NULL ref", {"ref_": None}), ("NULL output", {"out": None}),
                          ("NULL workspace", {"work": None}), ("S=0", {"S_": 0}), ("K=0", {"K_": 0}), ("m=0", {"m": 0}),
                          ("m=4", {"m": 4}), ("S=65536", {"S_": 65536}), ("short workspace", {"nbytes": 255})):
            fn(label, **kw)
    boxes("K=2049", K_=2049, J=4096)
    boxes("J=4097", J=4097)
    boxes("J one short", J=2 * K - 2)
    boxes("J one short at m=2", m=2, J=K - 1)
    front("K=16385", K_=16385)
    return calls


def record():
    """What the fixture holds, from the library that is loaded."""
    lib = _lib().load()
    sizes = {name: [list(a) + [int(getattr(lib, name)(*a))] for a in args] for name, args in QUERIES.items()}
    refused = []
    for label, thunk in refusals():
        status = int(thunk())
        refused.append([label, status, lib.dkg_last_error().decode()])
    return {"workspace": sizes, "refusals": refused}


def _golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acq_host.json")) as f:
        return json.load(f)


def test_workspace_sizes_are_the_recorded_ones():
    want, got = _golden()["workspace"], record()["workspace"]
    assert sorted(want) == sorted(QUERIES)
    for name in QUERIES:
        assert len(QUERIES[name]) >= 12 and any(row[-1] == 0 for row in want[name]) and any(row[-1] > 0 for row in want[name])
        assert got[name] == want[name], name


def test_refusals_are_the_recorded_ones():
    L = _lib()
    want, got = _golden()["refusals"], record()["refusals"]
    assert [w[0] for w in want] == [g[0] for g in got]
    for w, g in zip(want, got):
        assert w[1] != L.DKG_OK and w[1] in (L.DKG_ERR_ARG, L.DKG_ERR_UNSUPPORTED, L.DKG_ERR_WORKSPACE), w
        assert g == w, (w, g)
    text = " | ".join(w[2] for w in want)
    for pinned in ("state 2 output 1: kernel id 7", "m = 2 and m = 3", "not initialised", "output 1: NULL pointer"):
        assert pinned in text

