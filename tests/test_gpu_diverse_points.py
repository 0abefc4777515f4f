"""The filtered round and the efficacy measure over a batch of LP points on the device (sdpcut_round_csr_points_diverse,
sdpcut_efficacy_points) against the single-point calls on a SECOND handle with the same instance, candidates, networks, objective
and weight: round_csr_diverse(point p, ...) -- after set_box where the batch has boxes -- and set_point + score(EIG | EFF) +
get_efficacy.  Every comparison is np.array_equal on every field (scores as bit patterns): the claim is identity with the
single-point path, which tests/test_gpu_diverse.py and tests/test_gpu_efficacy.py tie to the numpy twins.  Lists, points and cases:
tests/diverse_points_cases.py, whose premises tests/test_diverse_points_cpu.py checks without a device."""
import ctypes

import numpy as np
import pytest

import diverse_points_cases as dc

pytestmark = pytest.mark.gpu

EIG, NN, EFF = 1, 2, 8
FLAGS = {1: EIG, 2: NN, 4: EIG | NN, 6: EIG | EFF}
ARRAYS = ("idx", "score", "lam", "ks", "set_inds", "row_entry", "indptr", "indices", "values", "rhs")
MPS = (0.0, 0.5, 0.9, 1.0)
MARGIN = 1e-12


@pytest.fixture(scope="module")
def pair():
    """(batched handle, single-point handle) with the four shipped networks"""
    import sdpcutsel_via_nn_amd as pkg
    scs = []
    for _ in range(2):
        sc = pkg.Scorer(0)
        sc.set_builtin_networks(5)
        scs.append(sc)
    yield tuple(scs)
    for sc in scs:
        sc.close()


def bind(pair, name, count=None, obj=True, w=dc.EFF_W):
    """the list (its first ``count`` candidates) on both handles, with the instance's LP objective and the weight -> (n, N)"""
    n, Q, S, ks, lpobj = dc.load(name)
    if count is not None:
        S, ks = S[:count], ks[:count]
    for sc in pair:
        sc.drop_pending()
        sc.set_instance(n, Q)      # (clears a box)
        sc.set_candidates(S, ks)
        sc.set_objective(lpobj if obj else None)
        sc.set_efficacy_weight(w)
    return n, S.shape[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_round(got, want, what=""):
    """every field of a filtered round: the arrays (dtype, shape -- n_out, n_rows and nnz are their lengths -- and values, the
    floating-point ones as bit patterns), n_total, new_strat, counters, info"""
    assert set(got) == set(want), what
    for f in ARRAYS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
        if got[f].dtype == np.float64:
            assert np.array_equal(bits(got[f]), bits(want[f])), (what, f)
        else:
            assert np.array_equal(got[f], want[f]), (what, f)
    assert (got["n_total"], got["new_strat"], got["counters"]) == (want["n_total"], want["new_strat"], want["counters"]), what
    assert got["info"] == want["info"], (what, got["info"], want["info"])


def single_rounds(single, pts, strat, sel, mp, pool, boxes=None):
    out = []
    for p in range(len(pts)):
        if boxes is not None:
            single.set_box(boxes[p, 0], boxes[p, 1])
        out.append(single.round_csr_diverse(pts[p], strat, sel, mp, pool_size=pool, copy=True))
    if boxes is not None:
        single.clear_box()
    return out


def fast_points(sc):
    from sdpcutsel_via_nn_amd import _capi
    return sc.get_stat(_capi.STAT_DIVERSE_POINTS_FAST), sc.get_stat(_capi.STAT_POINTS_REDONE)


def compare_batches(batch, single, pts, strat, sel, mp, pool, sizes=(1, 3, 8), boxes=None, route="fast", what=""):
    """the batch of the first P points, P in ``sizes``, against the single-point rounds -> those rounds"""
    ref = single_rounds(single, pts, strat, sel, mp, pool, boxes)
    for P in sizes:
        f0, r0 = fast_points(batch)
        got = batch.round_csr_points_diverse(pts[:P], strat, sel, mp, pool_size=pool, boxes=None if boxes is None else boxes[:P])
        assert len(got) == P
        for p in range(P):
            assert_same_round(got[p], ref[p], (what, strat, sel, pool, mp, P, p))
        f1, r1 = fast_points(batch)
        if route == "fast":
            assert f1 - f0 == P - (r1 - r0) and r1 - r0 <= P // 2, (what, "not the one-wait route", f1 - f0, r1 - r0)
        else:
            assert (f1 - f0, r1 - r0) == (0, 0), (what, "not the loop")
        assert batch.box is None and batch.get_stat(3) == 0      # no box, nothing scored: no current point
    return ref


# ------------------------------------------------------------------------------------------ 1. efficacy over points
def efficacy_points_of(name):
    """eight points: six of the list's, one with half of the variables at zero (candidates inside them: lambda_min = 0) and the origin"""
    n = dc.load(name)[0]
    L = n * (n + 1) // 2
    pts = dc.points(name)[[0, 1, 2, 4, 6, 7]]
    half = dc.points(name)[7].copy()
    iu = np.triu_indices(n)
    dead = np.arange(n) % 2 == 0
    half[:L][dead[iu[0]] | dead[iu[1]]] = 0.0
    half[L:][dead] = 0.0
    return np.concatenate([pts, half[None], np.zeros((1, L + n))])


@pytest.mark.parametrize("count", [1, 63, 64, 65, 1051])
def test_efficacy_points(pair, count):
    batch, single = pair
    pts = efficacy_points_of("spar020")
    zeros_seen = False
    for obj, w in ((False, 0.0), (False, 0.1), (True, 0.0), (True, 0.1)):
        n, N = bind(pair, "spar020", count, obj, w)
        ref = []
        for p in range(8):
            single.set_point(pts[p])
            single.score(EIG | EFF)
            ref.append(single.get_efficacy())
            zeros_seen = zeros_seen or bool(np.any(single.get_scores(obj=False)[0] == 0.0))
        for P in (1, 3, 8):
            got = batch.efficacy_points(pts[:P] if P < 8 else pts)
            for j, name in enumerate(("eff", "objpar", "escore")):
                assert got[j].shape == (P, N)
                for p in range(P):
                    assert np.array_equal(bits(got[j][p]), bits(ref[p][j])), (count, obj, w, P, p, name)
            assert batch.get_stat(3) == 0 and batch.box is None
        last = batch.efficacy_points(pts[5:])      # (the points with lambda = 0 candidates in a batch of their own)
        assert not np.any(np.signbit(last[0][last[0] == 0.0]))
        if not obj:
            assert np.all(got[1] == 0.0)
    print("lambda_min == 0.0 exactly seen on the single-point handle:", zeros_seen)      # (the origin, the dead half)


# ------------------------------------------------------------------------------------------ 2. the one-wait route
def pool_at(single, strat, sel, pool, vv):
    """the pool of a round at vv as the single-point handle ranks it, with its rows -> (ids, Sp, kp, coef, eligible)"""
    from sdpcutsel_via_nn_amd import diversity
    single.set_point(vv)
    single.score(FLAGS[strat])
    ids = single.rank(strat, sel, max_out=pool)[0]
    loc = ids - single.base
    lam, coef, _, _, kk = single.cut_rows(loc)
    S, ks = single.get_candidates(loc)
    return ids, S, kk, coef, diversity.eligible_rows(lam, kk, coef)


def check_invariants(single, pts, strat, sel, pool, mps_rounds):
    """every returned row set passes the walk's invariant checker (diversity.check_walk) at its max_parallel"""
    from sdpcutsel_via_nn_amd import diversity
    for p in range(len(pts)):
        ids, Sp, kp, coef, el = pool_at(single, strat, sel, pool, pts[p])
        cos = diversity.pair_cosines(Sp, kp, coef) if ids.shape[0] else None
        for mp, rs in mps_rounds:
            r = rs[p]
            assert r["info"]["pool"] == ids.shape[0]
            if ids.shape[0] == 0:
                assert r["idx"].shape[0] == 0
                continue
            pos = {int(g): i for i, g in enumerate(ids)}
            at = np.array([pos[int(g)] for g in r["idx"]], dtype=np.int64)
            assert np.array_equal(at, np.sort(at)) and np.unique(at).shape[0] == at.shape[0]      # rank order, nobody twice
            keep = np.zeros(ids.shape[0], dtype=bool)
            keep[at] = True
            assert diversity.check_walk(Sp, kp, coef, el, sel, mp, keep, margin=MARGIN, examined=r["info"]["examined"], cos=cos)
            i = r["info"]
            assert i["examined"] == keep.sum() + i["skipped_nonviolated"] + i["rejected_parallel"]
            assert r["rhs"].shape[0] == r["idx"].shape[0] and np.array_equal(r["row_entry"], np.arange(r["idx"].shape[0]))


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: "%s-s%d-%d-%d" % c)
def test_fast_route(pair, case):
    """P = 1, 3, 8 at four thresholds; at 0.5 the twins promise rejections (and, strategies 2, 4, 6, entries that are not violated)"""
    batch, single = pair
    name, strat, sel, pool = case
    bind(pair, name)
    pts = dc.points(name)
    by_mp = []
    for mp in MPS:
        ref = compare_batches(batch, single, pts, strat, sel, mp, pool, what=name)
        by_mp.append((mp, ref))
        if mp == dc.MP:
            assert max(r["info"]["rejected_parallel"] for r in ref) > 0
            assert strat == 1 or max(r["info"]["skipped_nonviolated"] for r in ref) > 0
        if mp == 1.0:
            assert all(r["info"]["rejected_parallel"] == 0 for r in ref)
    check_invariants(single, pts, strat, sel, pool, by_mp)


def test_walk_ends_at_a_block_end_and_inside_a_block(pair):
    batch, single = pair
    bind(pair, "spar040")
    got = batch.round_csr_points_diverse(dc.points("spar040"), 1, 20, dc.MP, pool_size=65, copy=True)
    info = [r["info"] for r in got]
    assert info[1]["examined"] == 64 and got[1]["idx"].shape[0] == 20 and info[1]["pool"] == 65      # the quota fills with entry 63
    assert info[3]["examined"] % 64 != 0 and got[3]["idx"].shape[0] == 20 and info[3]["examined"] < info[3]["pool"]
    assert info[7] == dict(pool=0, examined=0, skipped_nonviolated=0, rejected_parallel=0) and got[7]["indptr"].tolist() == [0]


@pytest.mark.parametrize("name,strat", [(n, s) for n in ("spar020", "spar040") for s in (1, 2, 6)])
def test_pools_at_block_edges(pair, name, strat):
    """pools of 1, 63, 64 and 65 entries, sel < pool and sel = pool; and lists shorter than the pool asked for"""
    batch, single = pair
    bind(pair, name)
    pts = dc.points(name)
    for lst, s, sel, pool in dc.EDGE_CASES:
        if (lst, s) == (name, strat):
            compare_batches(batch, single, pts, strat, sel, dc.MP, pool, sizes=(8,), what="edge")
    for count in (63, 65):      # pool = min(pool_size, N) = the whole sub-list
        bind(pair, name, count)
        compare_batches(batch, single, pts, strat, 40, dc.MP, 512, sizes=(3,), what="sub-list %d" % count)
        compare_batches(batch, single, pts, 4, 512, dc.MP, 512, sizes=(3,), what="sub-list %d" % count)


def test_256_points(pair):
    batch, single = pair
    bind(pair, "spar040")
    pts = dc.many_points("spar040", 256)
    compare_batches(batch, single, pts, 2, 30, dc.MP, 129, sizes=(256,), what="256 points")


def test_vertex_point_in_a_batch(pair):
    """the McCormick vertex (tied scores: selections that may declare themselves void and are redone) next to ordinary points"""
    batch, single = pair
    n, N = bind(pair, "spar020")
    pts = dc.points("spar020")[:4].copy()
    pts[2] = dc.mccormick_vertex(n, dc.load("spar020")[1])
    for strat, sel, pool in ((1, 40, 129), (4, 129, 129), (2, 50, 129), (6, 30, 129)):
        ref = single_rounds(single, pts, strat, sel, dc.MP, pool)
        got = batch.round_csr_points_diverse(pts, strat, sel, dc.MP, pool_size=pool)
        for p in range(4):
            assert_same_round(got[p], ref[p], ("vertex", strat, p))


# ------------------------------------------------------------------------------------------ 3. the loop
@pytest.mark.parametrize("strat", [1, 2, 4, 6])
def test_loop_route(pair, strat):
    """pool 513, a list of 4097 candidates, and the combined strategy with sel < pool: the single-point call per point inside"""
    from sdpcutsel_via_nn_amd import harness, synthetic
    batch, single = pair
    bind(pair, "spar020")
    pts = dc.points("spar020")[[0, 3]]
    compare_batches(batch, single, pts, strat, 100, dc.MP, 513, sizes=(2,), route="loop", what="pool 513")
    if strat == 4:
        compare_batches(batch, single, pts, 4, 50, dc.MP, 129, sizes=(2,), route="loop", what="combined, sel < pool")
    n = 40
    Q_arr, _, _ = synthetic.make_instance(n, 7)
    for sc in pair:
        sc.drop_pending()
        sc.set_instance(n, np.asarray(Q_arr, dtype=np.float64))
        sc.set_candidates_philox(3, 4097, seed=7)
        sc.set_objective(None)
    big = np.stack([harness.random_mccormick_point(n, np.random.default_rng(40 + p)) for p in range(2)])
    compare_batches(batch, single, big, strat, 100, dc.MP, 400, sizes=(2,), route="loop", what="N 4097")


# ------------------------------------------------------------------------------------------ 4. a box per point
@pytest.mark.parametrize("strat,sel,pool,route", [(2, 50, 129, "fast"), (4, 129, 129, "fast"), (2, 100, 513, "loop"), (4, 100, 513, "loop")])
def test_boxed(pair, strat, sel, pool, route):
    batch, single = pair
    bind(pair, "spar020")
    boxes, pts = dc.boxes_and_points("spar020", 8)
    assert np.all(boxes[:, 1] - boxes[:, 0] >= 2.0 ** -10)
    ref = compare_batches(batch, single, pts, strat, sel, dc.MP, pool, sizes=(1, 3, 8) if route == "fast" else (3,), boxes=boxes, route=route,
                          what="boxed")
    plain = single_rounds(single, pts, strat, sel, dc.MP, pool)
    assert any(not np.array_equal(a["idx"], b["idx"]) for a, b in zip(ref[1:], plain[1:]))      # the boxes matter
    assert_same_round(ref[0], plain[0], "the unit box")


@pytest.mark.parametrize("strat,sel,pool", [(1, 40, 129), (6, 30, 129), (1, 100, 513)])
def test_boxes_change_nothing_for_strategies_1_and_6(pair, strat, sel, pool):
    batch, single = pair
    bind(pair, "spar020")
    boxes, pts = dc.boxes_and_points("spar020", 3)
    plain = batch.round_csr_points_diverse(pts, strat, sel, dc.MP, pool_size=pool, copy=True)
    boxed = batch.round_csr_points_diverse(pts, strat, sel, dc.MP, pool_size=pool, boxes=boxes, copy=True)
    ref = single_rounds(single, pts, strat, sel, dc.MP, pool, boxes)
    for p in range(3):
        assert_same_round(boxed[p], plain[p], ("boxed = unboxed", strat, p))
        assert_same_round(boxed[p], ref[p], ("boxed = single", strat, p))
    assert batch.box is None


# ------------------------------------------------------------------------------------------ 5. no filter = the plain batch
@pytest.mark.parametrize("strat", [1, 2, 4])
def test_no_filter_equals_the_plain_batch(pair, strat):
    """max_parallel = 1, pool = sel: round_csr_points restricted to its cut-yielding entries"""
    batch, _ = pair
    bind(pair, "spar020")
    pts = dc.points("spar020")
    for sel in (100, 129):
        plain = batch.round_csr_points(pts, strat, sel, copy=True)
        got = batch.round_csr_points_diverse(pts, strat, sel, 1.0, pool_size=sel, copy=True)
        for a, d in zip(plain, got):
            e = a["row_entry"]
            for f in ("idx", "score", "lam", "ks", "set_inds"):
                assert d[f].dtype == a[f].dtype and np.array_equal(d[f], a[f][e]), (sel, f)
            for f in ("indptr", "indices", "values", "rhs"):
                assert d[f].dtype == a[f].dtype and np.array_equal(d[f], a[f]), (sel, f)
            assert np.array_equal(d["row_entry"], np.arange(e.shape[0], dtype=np.int32))
            assert (d["n_total"], d["new_strat"], d["counters"]) == (a["n_total"], a["new_strat"], a["counters"])
            w = a["idx"].shape[0]
            assert d["info"] == dict(pool=w, examined=w, skipped_nonviolated=w - e.shape[0], rejected_parallel=0)


# ------------------------------------------------------------------------------------------ 6. state and refusals
def test_handle_state_after_the_call(pair):
    batch, single = pair
    n, N = bind(pair, "spar020")
    pts = dc.points("spar020")
    boxes, bpts = dc.boxes_and_points("spar020", 3)
    for kw in (dict(points=pts, strat=6, sel_size=30, pool_size=129), dict(points=bpts, strat=4, sel_size=129, pool_size=129, boxes=boxes),
               dict(points=pts[:2], strat=2, sel_size=100, pool_size=513)):
        batch.round_csr_points_diverse(max_parallel=dc.MP, **kw)
        assert batch.box is None and batch.get_stat(3) == 0
        with pytest.raises(Exception):
            batch.get_scores()      # no current point
        with pytest.raises(Exception):
            batch.get_efficacy()
        for strat in (4, 1, 2):
            got, want = batch.round_csr(strat, 60, point=pts[1], copy=True), single.round_csr(strat, 60, point=pts[1], copy=True)
            for f in ARRAYS:
                assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (strat, f)
            assert (got["n_total"], got["new_strat"], got["counters"]) == (want["n_total"], want["new_strat"], want["counters"])
        batch.round_csr_points_diverse(max_parallel=dc.MP, **kw)
        for strat in (4, 2):
            got, want = batch.round_csr_points(pts[:3], strat, 60, copy=True), single.round_csr_points(pts[:3], strat, 60, copy=True)
            for g, w in zip(got, want):
                for f in ARRAYS:
                    assert np.array_equal(g[f], w[f]), (strat, f)
                assert (g["n_total"], g["new_strat"], g["counters"]) == (w["n_total"], w["new_strat"], w["counters"])
    batch.efficacy_points(pts[:3])
    assert batch.box is None and batch.get_stat(3) == 0
    got, want = batch.round_csr_diverse(pts[0], 6, 30, dc.MP, copy=True), single.round_csr_diverse(pts[0], 6, 30, dc.MP, copy=True)
    assert_same_round(got, want, "strategy 6 after efficacy_points")


def test_refusals_leave_the_handle_unchanged(pair):
    batch, _ = pair
    n, N = bind(pair, "spar020")
    pts = np.ascontiguousarray(dc.points("spar020")[:2])
    lib, h = batch._lib, batch._h
    dp = ctypes.POINTER(ctypes.c_double)
    out, info = (_capi_mod().RoundCsr * 2)(), (_capi_mod().DiverseInfo * 2)()
    L = n * (n + 1) // 2
    boxes = np.zeros((2, 2, n))
    boxes[:, 1] = 1.0
    ld = pts.shape[1]

    def call(strat=1, sel=10, pool=40, mp=0.5, bx=None, P=2, point_ld=ld):
        lb = ub = None
        if bx is not None:
            lb, ub = bx.ctypes.data_as(dp), ctypes.cast(ctypes.c_void_p(bx.ctypes.data + 8 * n), dp)
        return lib.sdpcut_round_csr_points_diverse(h, P, pts.ctypes.data_as(dp), point_ld, lb, ub, 2 * n, strat, sel, pool, mp, out, info)

    def unchanged():
        """the point set before the refusals is still the current one, with its scores"""
        assert batch.get_stat(3) == EIG
        assert np.array_equal(bits(batch.get_scores(obj=False)[0]), bits(lam0))

    batch.set_point(pts[0])
    batch.score(EIG)
    lam0 = batch.get_scores(obj=False)[0]
    for kw in (dict(strat=0), dict(strat=3), dict(strat=5), dict(strat=104), dict(mp=-0.01), dict(mp=1.01), dict(mp=float("nan")), dict(sel=0),
               dict(pool=9), dict(pool=16385), dict(P=0), dict(P=257), dict(point_ld=ld - 1)):
        assert call(**kw) == -1, kw      # SDPCUT_EINVAL
        unchanged()
    assert lib.sdpcut_efficacy_points(h, 2, pts.ctypes.data_as(dp), ld, None, None, None) == -1
    assert lib.sdpcut_efficacy_points(h, 0, pts.ctypes.data_as(dp), ld, pts.ctypes.data_as(dp), None, None) == -1
    unchanged()
    # a bad box: the message names the point and the variable; nothing has changed
    bad = boxes.copy()
    bad[1, 1, 7] = bad[1, 0, 7] + 2.0 ** -11
    assert call(strat=2, bx=bad) == -1
    msg = lib.sdpcut_last_error(h).decode()
    assert "point 1" in msg and "variable 7" in msg, msg
    unchanged()
    # one of lb / ub missing
    assert lib.sdpcut_round_csr_points_diverse(h, 2, pts.ctypes.data_as(dp), ld, boxes.ctypes.data_as(dp), None, 2 * n, 2, 10, 40, 0.5, out, info) == -1
    unchanged()
    # a box of the handle's own: refused, and kept
    lb, ub = np.full(n, 0.25), np.full(n, 0.75)
    batch.set_box(lb, ub)
    batch.set_point(pts[0])
    batch.score(EIG)
    for bx in (None, boxes):
        assert call(strat=2, bx=bx) == -4      # SDPCUT_ESTATE
        assert lib.sdpcut_efficacy_points(h, 2, pts.ctypes.data_as(dp), ld, pts.ctypes.data_as(dp), None, None) == -4
        got = batch.box
        assert got is not None and np.array_equal(got[0], lb) and np.array_equal(got[1], ub)
        unchanged()
    batch.clear_box()
    # a round pending
    batch.round_csr_begin(1, 10, point=pts[0])
    assert call() == -4 and call(strat=2, bx=boxes) == -4
    assert lib.sdpcut_efficacy_points(h, 2, pts.ctypes.data_as(dp), ld, pts.ctypes.data_as(dp), None, None) == -4
    r = batch.round_csr_end()
    assert r["idx"].shape[0] == 10      # the pending round is still whole
    # exact heads on: a boxed batch is refused as sdpcut_set_box refuses it
    batch.set_option(_capi_mod().OPT_EXACT_HEAD, 1)
    try:
        assert call(strat=2, bx=boxes) == -4
    finally:
        batch.set_option(_capi_mod().OPT_EXACT_HEAD, 0)
    # and the call still works
    assert call() == 0 and call(strat=6, bx=boxes) == 0


def _capi_mod():
    from sdpcutsel_via_nn_amd import _capi
    return _capi


# ------------------------------------------------------------------------------------------ 7. the host layer above
def test_separate_points_with_the_filter(pair):
    """CutSolver.separate_points with max_parallel: per node the rows of the single-point filtered round, boxed and unboxed;
    max_parallel=None is the plain batched round"""
    import sdpcutsel_via_nn_amd as pkg
    batch, single = pair
    n, N = bind(pair, "spar020", obj=False, w=0.0)
    _, Q, S, ks, _ = dc.load("spar020")
    cs = pkg.CutSolver()
    sets = [[int(v) for v in S[t, :ks[t]]] for t in range(N)]
    agg = [(s, [n * s[a] - s[a] * (s[a] + 1) // 2 + s[b] for a in range(len(s)) for b in range(a, len(s))], None, None) for s in sets]
    cs.set_instance(n, Q, agg, dim=3)
    try:
        pts = dc.points("spar020")[:3]
        boxes, bpts = dc.boxes_and_points("spar020", 3)
        for strat, sel, factor in ((1, 40, 3), (2, 50, 2), (4, 100, 1), (6, 30, 4)):
            pool = min(max(int(factor * sel), sel), 16384)
            for use_boxes in (False, True):
                ref = single_rounds(single, bpts if use_boxes else pts, strat, sel, dc.MP, pool, boxes if use_boxes else None)
                nodes = cs.separate_points(strat, bpts if use_boxes else pts, sel, boxes=boxes if use_boxes else None, max_parallel=dc.MP,
                                           pool_factor=factor)
                assert len(nodes) == 3
                for p, (csr, n_total, new_strat, counters) in enumerate(nodes):
                    assert (n_total, new_strat, counters) == (ref[p]["n_total"], ref[p]["new_strat"], ref[p]["counters"])
                    for got, f in zip(csr, ("indptr", "indices", "values", "rhs")):
                        assert np.array_equal(got, ref[p][f]), (strat, use_boxes, p, f)
        plain = single.round_csr_points(pts, 4, 100, copy=True)
        for p, (csr, n_total, new_strat, counters) in enumerate(cs.separate_points(4, pts, 100)):
            assert (n_total, new_strat, counters) == (plain[p]["n_total"], plain[p]["new_strat"], plain[p]["counters"])
            for got, f in zip(csr, ("indptr", "indices", "values", "rhs")):
                assert np.array_equal(got, plain[p][f]), (p, f)
        with pytest.raises(ValueError):
            cs.separate_points(3, pts, 40, max_parallel=dc.MP)
        with pytest.raises(ValueError):
            cs.separate_points(1, pts, 40, max_parallel=1.5)
    finally:
        for bnd in cs._gpu_bindings.values():
            bnd.scorer.close()
