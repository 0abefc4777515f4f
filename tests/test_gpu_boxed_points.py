"""Batched rounds with a node box per point on the device: sdpcut_score_points_boxed / sdpcut_round_csr_points_boxed against the
single-point path on a SECOND handle with the same instance, candidates and networks -- set_box, then set_point + score +
get_scores or round_csr(point=).  Every comparison is np.array_equal on every field: the claim is identity with the single-point
boxed path, which test_gpu_node_box.py ties to the numpy twin.  Instances, boxes and points: tests/nodebox_cases.py (box 0 of
every batch is the unit box)."""
import numpy as np
import pytest

import nodebox_cases as nc

pytestmark = pytest.mark.gpu

EIG, NN = 1, 2
ARRAYS = ("idx", "score", "lam", "ks", "set_inds", "row_entry", "indptr", "indices", "values", "rhs")
N_VARS = 20      # of the synthetic lists
P_MAX = 17


@pytest.fixture(scope="module")
def pair():
    """(batched handle, single-point handle) with the four shipped networks (single_scores / single_rounds leave the single-point
    handle without a box)"""
    import sdpcutsel_via_nn_amd as pkg
    scs = []
    for _ in range(2):
        sc = pkg.Scorer(0)
        sc.set_builtin_networks(5)
        scs.append(sc)
    yield tuple(scs)
    for sc in scs:
        sc.close()


_COVERS = {}


def cover(case):
    from sdpcutsel_via_nn_amd import _capi
    if case not in _COVERS:
        inst, dim = nc.instance(case)
        S, ks, _ = _capi.enumerate_cover(inst["adj"], dim)
        _COVERS[case] = (inst["nb_vars"], np.asarray(inst["Q_arr"], dtype=np.float64), np.ascontiguousarray(S), np.ascontiguousarray(ks))
    return _COVERS[case]


def bind(pair, n, Q_arr, S, ks):
    for sc in pair:
        sc.drop_pending()
        sc.set_instance(n, np.asarray(Q_arr, dtype=np.float64))      # (clears a box)
        sc.set_candidates(S, ks)


def bind_case(pair, case):
    n, Q, S, ks = cover(case)
    if case == "spar020":
        assert S.shape[0] == 1051 and set(np.unique(ks).tolist()) == {3}
    else:
        assert S.shape[0] == 142 and set(np.unique(ks).tolist()) == {2, 3, 4, 5}
    bind(pair, n, Q, S, ks)
    return n, S.shape[0]


def synthetic_list(k, N, seed=7):
    from sdpcutsel_via_nn_amd import synthetic
    Q_arr, _, rng = synthetic.make_instance(N_VARS, seed)
    s = synthetic.random_index_sets(N_VARS, k, N, rng)
    pad = np.full((N, 5), -1, dtype=np.int32)
    pad[:, :k] = s
    return Q_arr, pad, np.full(N, k, dtype=np.int32)


def boxes_and_points(n, P, seed0):
    """P boxes (box 0: the unit box) and a McCormick-feasible point of each"""
    boxes = np.stack([np.stack((np.zeros(n), np.ones(n)))] + [np.stack(nc.random_box(n, seed0 + p)) for p in range(1, P)])
    pts = np.stack([nc.point_in_box(n, boxes[p, 0], boxes[p, 1], seed0 + p) for p in range(P)])
    return boxes, pts


def psd_point_in_box(n, lb, ub, seed):
    """X = x x^T at an x inside the box: nothing is violated there"""
    x = lb + (ub - lb) * np.random.default_rng(seed).uniform(0.1, 0.9, n)
    return np.concatenate([(x[:, None] * x[None, :])[np.triu_indices(n)], x])


def single_scores(single, boxes, pts, flags):
    """row p: set_box, set_point, score, get_scores on the single-point handle"""
    N = single.N
    e, o = np.empty((len(pts), N)), np.empty((len(pts), N))
    for p in range(len(pts)):
        single.set_box(boxes[p, 0], boxes[p, 1])
        single.set_point(pts[p])
        single.score(flags)
        ge, go = single.get_scores(eig=bool(flags & EIG), obj=bool(flags & NN))
        if flags & EIG:
            e[p] = ge
        if flags & NN:
            o[p] = go
    single.clear_box()
    return e, o


def single_rounds(single, boxes, pts, strat, sel):
    out = []
    for p in range(len(pts)):
        single.set_box(boxes[p, 0], boxes[p, 1])
        out.append(single.round_csr(strat, sel, point=pts[p], copy=True))
    single.clear_box()
    return out


def assert_same_round(got, want, what=""):
    """every field of a round: the arrays (dtype, shape -- n_out, n_rows and nnz are their lengths -- and values), n_total,
    new_strat, counters"""
    assert set(got) == set(want), what
    for f in ARRAYS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f]), (what, f)
    assert (got["n_total"], got["new_strat"], got["counters"]) == (want["n_total"], want["new_strat"], want["counters"]), what


def assert_same_bits(a, b, what=""):
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


# ------------------------------------------------------------------------------------------ 1. scores
@pytest.mark.parametrize("case", ["spar020", "mixed"])
def test_scores(pair, case):
    batch, single = pair
    n, N = bind_case(pair, case)
    boxes, pts = boxes_and_points(n, P_MAX, 500)
    for eig, obj in ((True, False), (False, True), (True, True)):
        flags = (EIG if eig else 0) | (NN if obj else 0)
        ref_e, ref_o = single_scores(single, boxes, pts, flags)
        for P in (1, 2, 3, P_MAX):
            e, o = batch.score_points(pts[:P], eig=eig, obj=obj, boxes=boxes[:P])
            assert (e is None) == (not eig) and (o is None) == (not obj)
            assert batch.box is None
            ue, uo = batch.score_points(pts[:P], eig=eig, obj=obj)      # no boxes: its unit-box row is the boxed call's
            if eig:
                assert_same_bits(e, ref_e[:P], (case, P, flags))
                assert_same_bits(e, ue, (case, P, flags))               # lambda_min knows no box
            if obj:
                assert_same_bits(o, ref_o[:P], (case, P, flags))
                assert_same_bits(o[0], uo[0], (case, P, flags))
                if P > 1:
                    assert not np.array_equal(o[1:], uo[1:])            # ... and the other rows are not


# ------------------------------------------------------------------------------------------ 2. strides
def test_strides_one_point_many_boxes_one_box_many_points(pair):
    from sdpcutsel_via_nn_amd import harness
    batch, single = pair
    n, N = bind_case(pair, "spar020")
    P = 5
    boxes, pts = boxes_and_points(n, P, 600)
    # the same LP point under P boxes: one lambda_min, P measures (a Q' stride of 0 would give P times the first box's)
    vv = harness.random_mccormick_point(n, np.random.default_rng(601))
    same = np.stack([vv] * P)
    ref_e, ref_o = single_scores(single, boxes, same, EIG | NN)
    e, o = batch.score_points(same, boxes=boxes)
    assert_same_bits(e, ref_e)
    assert_same_bits(o, ref_o)
    for p in range(1, P):
        assert np.array_equal(e[p], e[0]) and not np.array_equal(o[p], o[0]), p
    for strat in (2, 4):
        ref = single_rounds(single, boxes, same, strat, 100)
        got = batch.round_csr_points(same, strat, 100, boxes=boxes)
        for p in range(P):
            assert_same_round(got[p], ref[p], (strat, p))
    # the same box at P points
    one = np.stack([boxes[3]] * P)
    pts3 = np.stack([nc.point_in_box(n, boxes[3, 0], boxes[3, 1], 610 + p) for p in range(P)])
    ref_e, ref_o = single_scores(single, one, pts3, EIG | NN)
    e, o = batch.score_points(pts3, boxes=one)
    assert_same_bits(e, ref_e)
    assert_same_bits(o, ref_o)
    ref = single_rounds(single, one, pts3, 4, 100)
    got = batch.round_csr_points(pts3, 4, 100, boxes=one)
    for p in range(P):
        assert_same_round(got[p], ref[p], p)


@pytest.mark.parametrize("N", [1, 17, 4096])
def test_strides_tile_edges(pair, N):
    """synthetic 3-variable lists: one candidate, a tile of 16 plus one, the longest list of the one-wait route"""
    batch, single = pair
    Q_arr, S, ks = synthetic_list(3, N)
    bind(pair, N_VARS, Q_arr, S, ks)
    boxes, pts = boxes_and_points(N_VARS, 3, 700)
    for flags in (NN, EIG | NN):
        ref_e, ref_o = single_scores(single, boxes, pts, flags)
        e, o = batch.score_points(pts, eig=bool(flags & EIG), obj=True, boxes=boxes)
        if flags & EIG:
            assert_same_bits(e, ref_e, (N, flags))
        assert_same_bits(o, ref_o, (N, flags))
    sel = min(N, 100)
    for strat in (1, 2, 4):
        ref = single_rounds(single, boxes, pts, strat, sel)
        got = batch.round_csr_points(pts, strat, sel, boxes=boxes)
        for p in range(3):
            assert_same_round(got[p], ref[p], (N, strat, p))


# ------------------------------------------------------------------------------------------ 3. rounds
@pytest.mark.parametrize("case", ["spar020", "mixed"])
def test_rounds(pair, case):
    """strategies x head sizes x batch sizes.  Point 1 of every batch is a PSD point inside its box: no violated candidate, hence
    no strong one, so the combined strategy visits every entry there; the others are ordinary points, which at sel_size = 1 are in
    the strong regime -- both regimes of the per-point strong count in one batch."""
    from sdpcutsel_via_nn_amd import _capi
    batch, single = pair
    n, N = bind_case(pair, case)
    boxes, pts = boxes_and_points(n, P_MAX, 800)
    pts[1] = psd_point_in_box(n, boxes[1, 0], boxes[1, 1], 801)
    redone0 = batch.get_stat(_capi.STAT_POINTS_REDONE)
    for strat in (1, 2, 4):
        for sel in (1, 100, 512):
            ref = single_rounds(single, boxes, pts, strat, sel)
            for P in (1, 3, P_MAX):
                got = batch.round_csr_points(pts[:P], strat, sel, boxes=boxes[:P])
                assert len(got) == P and batch.box is None
                for p in range(P):
                    assert_same_round(got[p], ref[p], (case, strat, sel, P, p))
            if strat == 4:
                assert ref[1]["counters"]["nb_violated"] == 0 == ref[1]["counters"]["strong"]      # fewer than any quota: every entry visited
            if strat == 4 and sel == 1:
                strong = [r["counters"]["strong"] for r in ref]
                print("strong by point:", strong, "new_strat:", [r["new_strat"] for r in ref])
                assert strong[0] == 1 and strong[2] == 1      # the scan stopped at its quota: the strong regime
    print("points redone:", batch.get_stat(_capi.STAT_POINTS_REDONE) - redone0)


def test_rounds_256_points(pair):
    batch, single = pair
    n, N = bind_case(pair, "spar020")
    P = 256
    boxes, pts = boxes_and_points(n, P, 900)
    ref = single_rounds(single, boxes, pts, 4, 100)
    got = batch.round_csr_points(pts, 4, 100, boxes=boxes)
    assert len(got) == P
    for p in range(P):
        assert_same_round(got[p], ref[p], p)
    with pytest.raises(ValueError):
        batch.round_csr_points(np.concatenate([pts, pts[:1]]), 4, 100, boxes=np.concatenate([boxes, boxes[:1]]))


# ------------------------------------------------------------------------------------------ 4. loop route
@pytest.mark.parametrize("N,sel", [(4097, 100), (4096, 513)])
def test_loop_route(pair, N, sel):
    batch, single = pair
    Q_arr, S, ks = synthetic_list(3, N)
    bind(pair, N_VARS, Q_arr, S, ks)
    boxes, pts = boxes_and_points(N_VARS, 3, 1000)
    for strat in (1, 2, 4):
        ref = single_rounds(single, boxes, pts, strat, sel)
        got = batch.round_csr_points(pts, strat, sel, boxes=boxes, copy=True)
        for p in range(3):
            assert_same_round(got[p], ref[p], (N, sel, strat, p))
        assert batch.box is None


# ------------------------------------------------------------------------------------------ 5. state
def test_state_after_a_boxed_call(pair):
    from sdpcutsel_via_nn_amd import _capi
    batch, single = pair
    n, N = bind_case(pair, "spar020")
    boxes, pts = boxes_and_points(n, 4, 1100)
    before = batch.round_csr_points(pts[:3], 4, 100, copy=True)
    for call in (lambda: batch.round_csr_points(pts[:3], 4, 100, boxes=boxes[:3]), lambda: batch.score_points(pts[:3], boxes=boxes[:3])):
        batch.set_point(pts[3])
        batch.score(EIG | NN)
        call()
        assert batch.box is None
        with pytest.raises(_capi.SdpCutError, match="not scored"):
            batch.get_scores()
        with pytest.raises(_capi.SdpCutError, match="set_point first"):      # SDPCUT_ESTATE: no current point
            batch.score(EIG)
        after = batch.round_csr_points(pts[:3], 4, 100, copy=True)
        for p in range(3):
            assert_same_round(after[p], before[p], p)
    # a handle with a box of its own: refused, and the box stays
    lb, ub = nc.random_box(n, 1111)
    batch.set_box(lb, ub)
    try:
        with pytest.raises(_capi.SdpCutError, match="node box is set"):
            batch.round_csr_points(pts[:3], 4, 100, boxes=boxes[:3])
        with pytest.raises(_capi.SdpCutError, match="node box is set"):
            batch.score_points(pts[:3], boxes=boxes[:3])
        got = batch.box
        assert got is not None and np.array_equal(got[0], lb) and np.array_equal(got[1], ub)
    finally:
        batch.clear_box()
    # a bad box at point 2 of 3: refused before anything changes -- by the Python check, and by the library behind it
    bad = boxes[:3].copy()
    bad[2, 1, 5] = bad[2, 0, 5] + 2.0 ** -11
    batch.set_point(pts[3])
    batch.score(EIG)
    with pytest.raises(ValueError, match=r"point 2\b"):
        batch.round_csr_points(pts[:3], 4, 100, boxes=bad)
    import ctypes
    dp = ctypes.POINTER(ctypes.c_double)
    p3 = np.ascontiguousarray(pts[:3])
    out = (_capi.RoundCsr * 3)()
    e = np.empty((3, N))
    args = (batch._h, 3, p3.ctypes.data_as(dp), p3.shape[1], bad.ctypes.data_as(dp), ctypes.cast(ctypes.c_void_p(bad.ctypes.data + 8 * n), dp), 2 * n)
    assert batch._lib.sdpcut_round_csr_points_boxed(*args, 4, 100, out) == -1
    msg = batch._lib.sdpcut_last_error(batch._h)
    assert b"point 2" in msg and b"variable 5" in msg, msg
    assert batch._lib.sdpcut_score_points_boxed(*args, EIG, e.ctypes.data_as(dp), None) == -1
    assert b"point 2" in batch._lib.sdpcut_last_error(batch._h)
    assert batch._lib.sdpcut_round_csr_points_boxed(*args[:6], n - 1, 4, 100, out) == -1      # box_ld < n
    assert batch._lib.sdpcut_round_csr_points_boxed(*args[:4], None, args[5], 2 * n, 4, 100, out) == -1
    assert batch.get_stat(_capi.STAT_SCORED) == EIG and batch.box is None      # nothing changed: the point and its scores stand
    after = batch.round_csr_points(pts[:3], 4, 100, copy=True)
    for p in range(3):
        assert_same_round(after[p], before[p], p)
    # refusals shared with the unboxed call; reference-exact heads have no boxes
    for strat in (0, 3, -1, 5):
        with pytest.raises(ValueError, match="strategies 1 .*2 .*4"):
            batch.round_csr_points(pts[:3], strat, 100, boxes=boxes[:3])
    batch.set_option(_capi.OPT_EXACT_HEAD, 1)
    try:
        with pytest.raises(_capi.SdpCutError, match="EXACT_HEAD"):
            batch.round_csr_points(pts[:3], 4, 100, boxes=boxes[:3])
    finally:
        batch.set_option(_capi.OPT_EXACT_HEAD, 0)
    batch.round_csr_begin(1, 30, point=pts[2])
    with pytest.raises(_capi.SdpCutError, match="pending"):
        batch.round_csr_points(pts[:2], 1, 30, boxes=boxes[:2])
    with pytest.raises(_capi.SdpCutError, match="pending"):
        batch.score_points(pts[:2], boxes=boxes[:2])
    batch.round_csr_end()


# ------------------------------------------------------------------------------------------ 6. the solver classes
def test_separate_points_boxed_with_a_node_box_in_place(pair):
    import sdpcutsel_via_nn_amd as pkg
    batch, single = pair
    n, N = bind_case(pair, "spar020")
    _, Q, S, ks = cover("spar020")
    cs = pkg.CutSolver()
    sets = [[int(v) for v in S[t, :ks[t]]] for t in range(N)]
    agg = [(s, [n * s[a] - s[a] * (s[a] + 1) // 2 + s[b] for a in range(len(s)) for b in range(a, len(s))], None, None) for s in sets]
    cs.set_instance(n, Q, agg, dim=3)
    try:
        boxes, pts = boxes_and_points(n, 3, 1200)
        lb, ub = nc.random_box(n, 1210)
        cs.set_node_box(lb, ub)
        ref = single_rounds(single, boxes, pts, 4, 100)
        nodes = cs.separate_points(4, pts, 100, boxes=boxes)
        assert len(nodes) == 3
        for p, (csr, n_total, new_strat, counters) in enumerate(nodes):
            assert (n_total, new_strat, counters) == (ref[p]["n_total"], ref[p]["new_strat"], ref[p]["counters"])
            for got, f in zip(csr, ("indptr", "indices", "values", "rhs")):
                assert got.flags.owndata and np.array_equal(got, ref[p][f]), (p, f)
        # the solver's own box is on the handle again
        sc = cs._gpu_bind().scorer
        got = sc.box
        assert got is not None and np.array_equal(got[0], lb) and np.array_equal(got[1], ub)
        with pytest.raises(ValueError):
            cs.separate_points(4, pts, 100, boxes=boxes[:2])
        got = sc.box
        assert got is not None and np.array_equal(got[0], lb)
    finally:
        for bnd in cs._gpu_bindings.values():
            bnd.scorer.close()
