"""Triangle rounds with device rows, node boxes and many points (sdpcut_tri_round_csr, sdpcut_tri_round_csr_points) against the
numpy twin (sdpcutsel_via_nn_amd/triangles.py), byte for byte, and against tri_separate + the numpy build of
GpuCutSelectionMixin._separate_and_add_triangle (copied once, tests/tri_rows_numpy.py).

Shapes: n = 6 .. 12 with seeded patterns whose triple counts T = 1, 63, 64, 65 sit around a wave of 64 lanes and 4 T = 252 / 256 /
260 around 256, T = 220 (all triples of n = 12), and the golden covers (T = 1139, 1835: more than the 1024 threads of a workgroup,
two and more trips of every loop of tri_points_kernel).  Points: nothing violated; three of the four entries of EVERY triple
violated (the four facets of a triple cannot all be violated at once: v3 = -(v0 + v1 + v2) - 1); constant tables, whose keys are
all equal inside a density class, so that every threshold cuts through a mass of ties; random points; a NaN."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import nodebox_cases
from tri_rows_numpy import numpy_rows

pytestmark = pytest.mark.gpu

MAX_OUTS = (1, 2, 255, 256, 257, 4096)


def pattern_with(T):
    """a seeded sparsity pattern on n in 6 .. 12 variables with exactly T retained triples -> (n, adj)"""
    from sdpcutsel_via_nn_amd import triangles
    if T == 1:
        adj = np.zeros((6, 6), dtype=bool)
        adj[1, 3] = adj[3, 1] = adj[3, 4] = adj[4, 3] = True
        return 6, adj
    if T == 220:
        return 12, ~np.eye(12, dtype=bool)
    for seed in range(4000):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(8, 13))
        adj = np.triu(rng.uniform(size=(n, n)) < rng.uniform(0.3, 0.9), 1)
        adj = adj | adj.T
        if triangles.preprocess(adj)[0].shape[0] == T:
            return n, adj
    raise AssertionError("no pattern with %d triples" % T)


_INST = {}


def inst(T):
    """-> dict(n, adj, tri, dens) of the instance with T triples (1139 / 1835: the golden covers), built once"""
    from sdpcutsel_via_nn_amd import triangles
    if T not in _INST:
        if T in (1139, 1835):
            g = np.load(os.path.join(GOLDEN, "inst_tri.npz"))
            tag = "spar020_100_1" if T == 1139 else "spar040_030_1"
            n, adj = int(g[tag + "_nb_vars"]), g[tag + "_adj"] != 0
            pts = [np.array(g["%s_%s_0p1_vars" % (tag, k)], dtype=np.float64) for k in ("rnd", "mck")]
        else:
            n, adj = pattern_with(T)
            pts = None
        tri, dens = triangles.preprocess(adj)
        assert tri.shape[0] == T
        _INST[T] = dict(n=n, adj=adj, tri=tri, dens=dens, golden_points=pts)
    return _INST[T]


def const_point(n, x, X):
    L = n * (n + 1) // 2
    return np.concatenate([np.full(L, float(X)), np.full(n, float(x))])


def points_of(n, seed=0):
    """name -> LP point [X packed | x]"""
    rng = np.random.default_rng(100 + seed)
    L = n * (n + 1) // 2
    rnd = np.concatenate([rng.uniform(0, 1, L), rng.uniform(0, 1, n)])
    nan = rnd.copy()
    nan[L + n // 2] = np.nan
    nan[3] = np.nan
    return {"interior": const_point(n, 0.5, 0.25),      # every violation is -0.25
            "all": const_point(n, 0.0, 1.0),             # v0 = v1 = v2 = 1 in every triple
            "ties": const_point(n, 0.5, 0.75),           # v0 = v1 = v2 = 0.25: equal keys across every threshold
            "ties3": const_point(n, 0.5, 0.0),           # v3 = 0.5 in every triple
            "rnd": rnd, "nan": nan}


def scorer_for(I):
    from sdpcutsel_via_nn_amd import _capi
    sc = _capi.Scorer(0)
    sc.set_instance(I["n"], np.zeros(I["n"] * (I["n"] + 1) // 2))
    tri, dens = sc.tri_preprocess(I["adj"])
    assert np.array_equal(tri, I["tri"]) and np.array_equal(dens, I["dens"])
    return sc


def twin(I, vv, max_out, box=None):
    from sdpcutsel_via_nn_amd import triangles
    return triangles.round_csr(I["tri"], I["dens"], I["n"], vv, max_out, box=box)


def assert_same(got, want, what):
    from sdpcutsel_via_nn_amd import triangles
    assert got["n_rows"] == want["n_rows"] and got["n_violated"] == want["n_violated"], (what, got["n_rows"], want["n_rows"], got["n_violated"], want["n_violated"])
    for k in triangles.SAME_KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, k)


def check(I, vv, max_out, res, box=None):
    from sdpcutsel_via_nn_amd import triangles
    triangles.check_round(I["tri"], I["dens"], I["n"], vv, max_out, res, box=box)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 220])
def test_single_point_and_batch_equal_the_twin(T):
    """every point x every head length: the single call, the batch of all points (P = 6 here; 1, 2, 5 below) and the twin agree byte
    for byte; the checker holds on every result; counts: nothing / everything violated, max_out below, at and above n_violated and
    above 4 T"""
    I = inst(T)
    sc, batch = scorer_for(I), scorer_for(I)
    pts = points_of(I["n"], T)
    names = list(pts)
    assert twin(I, pts["interior"], 10)["n_violated"] == 0 and twin(I, pts["all"], 10)["n_violated"] == 3 * T
    assert twin(I, pts["nan"], 10)["n_violated"] <= twin(I, pts["rnd"], 10)["n_violated"]      # (a NaN violates nothing)
    nv = twin(I, pts["rnd"], 0)["n_violated"]
    for max_out in sorted(set(MAX_OUTS + (0, max(nv - 1, 0), nv, nv + 1, 4 * T, 4 * T + 1))):
        want = [twin(I, pts[k], max_out) for k in names]
        for k, w in zip(names, want):
            got = sc.tri_round_csr(max_out, point=pts[k])
            assert_same(got, w, (T, k, max_out, "single"))
            check(I, pts[k], max_out, got)
        got = batch.tri_round_csr_points(np.stack([pts[k] for k in names]), max_out)
        for k, g, w in zip(names, got, want):
            assert_same(g, w, (T, k, max_out, "batch"))
    sc.close(), batch.close()


@pytest.mark.parametrize("T", [1, 64, 65, 220])
def test_unboxed_equals_tri_separate_and_the_numpy_build(T):
    """without a box: entries and violations are tri_separate's on the same handle, the rows the numpy build's (int32 on the device)"""
    I = inst(T)
    sc = scorer_for(I)
    for name, vv in points_of(I["n"], T).items():
        for max_out in (2, 256, 4096):
            got = sc.tri_round_csr(max_out, point=vv, copy=True)
            ent, vio, nviol = sc.tri_separate(max_out)
            assert nviol == got["n_violated"] and ent.tobytes() == got["entry"].tobytes() and vio.tobytes() == got["viol"].tobytes(), (name, max_out)
            indptr, ind, val, rhs = numpy_rows(I["tri"], I["n"], ent)
            assert indptr.astype(np.int32).tobytes() == got["indptr"].tobytes() and ind.astype(np.int32).tobytes() == got["indices"].tobytes()
            assert val.tobytes() == got["values"].tobytes() and rhs.tobytes() == got["rhs"].tobytes(), (name, max_out)
    sc.close()


@pytest.mark.parametrize("P", [1, 2, 5])
@pytest.mark.parametrize("T", [63, 220])
def test_boxed_batch_equals_single_calls_and_the_twin(T, P):
    """a box per point: the batch = set_box + the single call per point on a fresh handle = the twin; unit boxes = no boxes"""
    I = inst(T)
    n = I["n"]
    boxes = np.array([nodebox_cases.random_box(n, 10 * T + p) for p in range(P)])
    pts = np.stack([nodebox_cases.point_in_box(n, boxes[p, 0], boxes[p, 1], 7 * T + p) if p % 2 == 0 else points_of(n, p)["rnd"] for p in range(P)])
    batch, single = scorer_for(I), scorer_for(I)
    unit = np.stack([np.stack([np.zeros(n), np.ones(n)])] * P)
    for max_out in (1, 255, 257, 4096):
        got = batch.tri_round_csr_points(pts, max_out, boxes=boxes, copy=True)
        for p in range(P):
            box = (boxes[p, 0], boxes[p, 1])
            assert_same(got[p], twin(I, pts[p], max_out, box), (T, P, p, max_out, "batch / twin"))
            check(I, pts[p], max_out, got[p], box=box)
            single.set_box(*box)
            assert_same(single.tri_round_csr(max_out, point=pts[p]), got[p], (T, P, p, max_out, "single / batch"))
            single.clear_box()
        assert batch.box is None
        plain = batch.tri_round_csr_points(pts, max_out, copy=True)
        for p, g in enumerate(batch.tri_round_csr_points(pts, max_out, boxes=unit)):
            assert_same(g, plain[p], (T, P, p, max_out, "unit boxes / no boxes"))
    single.set_box(np.zeros(n), np.ones(n))
    assert_same(single.tri_round_csr(300, point=pts[0]), twin(I, pts[0], 300), "unit box / no box, single")
    batch.close(), single.close()


def test_power_of_two_boxes_equal_the_stretched_instance():
    """l = 0, d = 2^-k: x' = x / d and X'_ij = X_ij / (d_i d_j) are exact, so the boxed round at (x, X) has the entries, violations,
    counts, columns and right-hand sides of the plain round at the stretched point, and its coefficients are that round's times the
    exact 1 / (d_i d_j), 1 / d_i"""
    I = inst(220)
    n, L = I["n"], I["n"] * (I["n"] + 1) // 2
    rng = np.random.default_rng(3)
    d = 2.0 ** -rng.integers(0, 4, n)
    i, j = np.triu_indices(n)
    st = points_of(n, 1)["rnd"]                       # the stretched point; the original one lies in the box
    vv = np.concatenate([st[:L] * (d[i] * d[j]), st[L:] * d])
    sc = scorer_for(I)
    plain = sc.tri_round_csr(100, point=st, copy=True)
    sc.set_box(np.zeros(n), d)
    boxed = sc.tri_round_csr(100, point=vv, copy=True)
    for k in ("entry", "viol", "indptr", "indices", "rhs"):
        assert plain[k].tobytes() == boxed[k].tobytes(), k
    assert plain["n_violated"] == boxed["n_violated"] > 100
    col = boxed["indices"].astype(np.int64)
    scale = np.where(col < L, 1.0 / (d[i] * d[j])[np.minimum(col, L - 1)], 1.0 / d[np.maximum(col - L, 0)])
    assert (plain["values"] * scale).tobytes() == boxed["values"].tobytes()
    sc.close()


def test_routes_agree_and_are_counted():
    """max_out = 4097 loops (the head no longer fits the workgroup's sort state), 4096 goes the one-wait way: on inputs with at most
    4096 violated entries both return the same bytes, on one with more the 4096 rows are a prefix; the statistic counts the points
    of the one-wait route only"""
    from sdpcutsel_via_nn_amd import _capi
    seen_longer = 0
    for T in (65, 1139, 1835):
        I = inst(T)
        sc = scorer_for(I)
        pts = np.stack(list(points_of(I["n"], 5).values())[:5])
        boxes = np.array([nodebox_cases.random_box(I["n"], 50 + p) for p in range(5)])
        for bx in (None, boxes):
            s0 = sc.get_stat(_capi.STAT_TRI_POINTS_FAST)
            fast = sc.tri_round_csr_points(pts, 4096, boxes=bx, copy=True)
            assert sc.get_stat(_capi.STAT_TRI_POINTS_FAST) == s0 + 5
            loop = sc.tri_round_csr_points(pts, 4097, boxes=bx, copy=True)
            assert sc.get_stat(_capi.STAT_TRI_POINTS_FAST) == s0 + 5
            for p in range(5):
                box = None if bx is None else (bx[p, 0], bx[p, 1])
                assert_same(loop[p], twin(I, pts[p], 4097, box), (T, p, "loop / twin"))
                if loop[p]["n_violated"] <= 4096:
                    assert_same(loop[p], fast[p], (T, p, "loop / fast"))
                else:
                    r = 4096
                    seen_longer += 1
                    assert fast[p]["n_rows"] == r and loop[p]["entry"][:r].tobytes() == fast[p]["entry"].tobytes()
                    assert loop[p]["values"][:loop[p]["indptr"][r]].tobytes() == fast[p]["values"].tobytes()
                    assert_same(fast[p], twin(I, pts[p], 4096, box), (T, p, "fast / twin"))
                    if seen_longer == 1:      # (the checker walks 4096 rows in Python: once)
                        check(I, pts[p], 4096, fast[p], box=box)
        sc.close()
    # T = 1835 at the constant points has 5505 violated entries, all ties inside a density class: the select pass, the collect of ties
    # in entry order and the sort run at the longest head the workgroup holds
    assert seen_longer >= 2


def test_state_after_the_calls():
    """the batch leaves no current point and no box; a plain round_csr after it equals the one of a fresh handle; the triangle calls
    work on a handle that holds a candidate list"""
    from sdpcutsel_via_nn_amd import _capi, synthetic
    I = inst(220)
    n = I["n"]
    wl = synthetic.make_workload(nb_vars=n, k=3, count=150, seed=3)

    def handle():
        sc = _capi.Scorer(0)
        sc.set_instance(n, wl["Q_arr"])
        sc.set_candidates(wl["set_inds"], wl["ks"])
        sc.tri_preprocess(I["adj"])
        return sc

    used, fresh = handle(), handle()
    pts = np.stack([points_of(n, s)["rnd"] for s in range(3)])
    boxes = np.array([nodebox_cases.random_box(n, s) for s in range(3)])
    got = used.tri_round_csr_points(pts, 100, boxes=boxes, copy=True)
    for p in range(3):
        assert_same(got[p], twin(I, pts[p], 100, (boxes[p, 0], boxes[p, 1])), p)
    assert used.box is None
    with pytest.raises(_capi.SdpCutError):
        used.tri_separate(10)      # no current point
    a, b = used.round_csr(1, 40, point=wl["vars_values"], copy=True), fresh.round_csr(1, 40, point=wl["vars_values"], copy=True)
    for k in ("idx", "score", "indptr", "indices", "values", "rhs"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    # ... and the single call after a round, then a round again
    assert_same(used.tri_round_csr(64, point=pts[0]), twin(I, pts[0], 64), "single after a round")
    assert_same(used.tri_round_csr(64), twin(I, pts[0], 64), "the current point")
    a = used.round_csr(1, 40, point=wl["vars_values"], copy=True)
    assert np.asarray(a["values"]).tobytes() == np.asarray(b["values"]).tobytes()
    used.close(), fresh.close()


def test_refusals():
    import ctypes
    from sdpcutsel_via_nn_amd import _capi
    I = inst(64)
    n = I["n"]
    m = n * (n + 1) // 2 + n
    sc = _capi.Scorer(0)
    sc.set_instance(n, np.zeros(m - n))
    rec, recs = _capi.TriCsr(), (_capi.TriCsr * 300)()
    pts = np.zeros((300, m))
    dp = pts.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    lib, h = sc._lib, sc._h
    assert lib.sdpcut_tri_round_csr(h, dp, 10, ctypes.byref(rec)) == -4                      # no preprocess
    assert lib.sdpcut_tri_round_csr_points(h, 2, dp, m, None, None, 10, recs) == -4
    sc.tri_preprocess(I["adj"])
    assert lib.sdpcut_tri_round_csr(h, None, 10, ctypes.byref(rec)) == -4                    # no current point
    assert lib.sdpcut_tri_round_csr(h, dp, 16385, ctypes.byref(rec)) == -1
    assert lib.sdpcut_tri_round_csr(h, dp, -1, ctypes.byref(rec)) == -1
    assert lib.sdpcut_tri_round_csr_points(h, 257, dp, m, None, None, 10, recs) == -1
    assert lib.sdpcut_tri_round_csr_points(h, 0, dp, m, None, None, 10, recs) == -1
    assert lib.sdpcut_tri_round_csr_points(h, 2, dp, m, None, None, 16385, recs) == -1
    assert lib.sdpcut_tri_round_csr_points(h, 2, dp, m - 1, None, None, 10, recs) == -1
    assert lib.sdpcut_tri_round_csr_points(h, 2, dp, m, dp, None, 10, recs) == -1           # one of lb / ub
    bad = np.zeros((2, n))
    bp = bad.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.sdpcut_tri_round_csr_points(h, 2, dp, m, bp, bp, 10, recs) == -1             # empty boxes
    sc.set_box(np.zeros(n), np.full(n, 0.5))
    assert lib.sdpcut_tri_round_csr_points(h, 2, dp, m, None, None, 10, recs) == -4         # a box of its own
    sc.clear_box()
    assert lib.sdpcut_tri_round_csr_points(h, 256, dp, m, None, None, 10, recs) == 0
    assert all(recs[p].n_violated == 0 and recs[p].n_rows == 0 for p in range(256))
    sc.close()


def test_a_void_selection_is_run_once_more():
    """the single call's answer to a selection that declared itself void (header word 3), made to run by SDPCUT_OPT_INJECT_GIVEUP at the
    selection site as the give-up tests do for tri_separate: one hit -> the same bytes after a second pass without the fused tail, counted
    as a fallback; two hits -> the call fails and says so; the handle serves the next call.  The loop route of the batch goes through it."""
    from sdpcutsel_via_nn_amd import _capi
    I = inst(1139)
    vv = I["golden_points"][1]
    want = twin(I, vv, 5000)
    assert want["n_violated"] > 257
    sc = scorer_for(I)
    assert_same(sc.tri_round_csr(5000, point=vv), want, "no injection")
    f0, i0 = sc.get_stat(_capi.STAT_SELECT_FALLBACKS), sc.get_stat(_capi.STAT_INJECTED)
    sc.set_option(_capi.OPT_INJECT_GIVEUP, _capi.inject_giveup(_capi.INJECT_SELECT))
    assert_same(sc.tri_round_csr(5000, point=vv), want, "one hit")
    assert (sc.get_stat(_capi.STAT_SELECT_FALLBACKS), sc.get_stat(_capi.STAT_INJECTED)) == (f0 + 1, i0 + 1)
    sc.set_option(_capi.OPT_INJECT_GIVEUP, _capi.inject_giveup(_capi.INJECT_SELECT, 0, 2))
    with pytest.raises(_capi.SdpCutError, match="tri_round_csr: selection void"):
        sc.tri_round_csr(5000, point=vv)
    assert sc.get_stat(_capi.STAT_INJECTED) == i0 + 3
    assert_same(sc.tri_round_csr(257, point=vv), twin(I, vv, 257), "after the failure")
    sc.set_option(_capi.OPT_INJECT_GIVEUP, _capi.inject_giveup(_capi.INJECT_SELECT))
    got = sc.tri_round_csr_points(np.stack([vv, vv]), 5000)      # (5000 > 4096: the loop route; the hit lands on point 0)
    assert_same(got[0], want, "batch, point 0")
    assert_same(got[1], want, "batch, point 1")
    assert sc.get_stat(_capi.STAT_INJECTED) == i0 + 4 and sc.get_stat(_capi.STAT_SELECT_FALLBACKS) == f0 + 3
    sc.close()


@pytest.mark.parametrize("T", [1139, 1835])
def test_golden_covers_at_depth_one_boxes(T):
    """the recorded LP points of spar020-100-1 and spar040-030-1 (tests/golden/inst_tri.npz) in the two depth-1 boxes of a branch at
    0.5 on the variable nearest to it, and at the root: batch = twin, and the checker on the heads of 257"""
    I = inst(T)
    n, L = I["n"], I["n"] * (I["n"] + 1) // 2
    pts, boxes = [], []
    for vv in I["golden_points"]:
        i = int(np.argmin(np.abs(vv[L:] - 0.5)))
        for side in (0, 1):
            lb, ub = np.zeros(n), np.ones(n)
            (ub if side == 0 else lb)[i] = 0.5
            pts.append(vv), boxes.append((lb, ub))
    pts, boxes = np.stack(pts), np.array(boxes)
    sc = scorer_for(I)
    for max_out in (257, 4096):
        root = sc.tri_round_csr_points(pts, max_out, copy=True)
        node = sc.tri_round_csr_points(pts, max_out, boxes=boxes, copy=True)
        for p in range(pts.shape[0]):
            assert_same(root[p], twin(I, pts[p], max_out), (T, p, max_out, "root"))
            assert_same(node[p], twin(I, pts[p], max_out, (boxes[p, 0], boxes[p, 1])), (T, p, max_out, "node"))
            if max_out == 257:
                check(I, pts[p], max_out, root[p])
                check(I, pts[p], max_out, node[p], box=(boxes[p, 0], boxes[p, 1]))
    sc.close()
