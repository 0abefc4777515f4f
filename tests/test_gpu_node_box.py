"""Node boxes on the device (sdpcut_set_box; csrc/box.hip): the transformed tables against the numpy twin, bit for bit, and the
semantics built on them -- the optimality measures of a boxed handle are those of a plain handle on the twin's tables, lambda_min
and the cut rows those of the original point.  Nothing here has a tolerance except the exact measure's certificate (its own
gap).  Instances, boxes and points: tests/nodebox_cases.py."""
from fractions import Fraction

import numpy as np
import pytest

import nodebox_cases as nc

pytestmark = pytest.mark.gpu

EIG, NN, SDP = 1, 2, 4
ARRAYS = ("idx", "score", "lam", "ks", "set_inds", "row_entry", "indptr", "indices", "values", "rhs")


def cover(case):
    from sdpcutsel_via_nn_amd import _capi
    inst, dim = nc.instance(case)
    S, ks, _ = _capi.enumerate_cover(inst["adj"], dim)
    return inst, np.ascontiguousarray(S), np.ascontiguousarray(ks)


_COVERS = {}


def bind(sc, case, Q=None):
    """the cover of `case` on the handle (its instance table Q, default the instance's) -> (n, Q_arr, S, ks)"""
    if case not in _COVERS:
        _COVERS[case] = cover(case)
    inst, S, ks = _COVERS[case]
    sc.drop_pending()
    Q_arr = np.asarray(inst["Q_arr"], dtype=np.float64) if Q is None else Q
    sc.set_instance(inst["nb_vars"], Q_arr)
    sc.set_candidates(S, ks)
    return inst["nb_vars"], Q_arr, S, ks


@pytest.fixture(scope="module")
def scorers():
    """two handles with the four shipped networks: the boxed one and a plain one to compare with"""
    import sdpcutsel_via_nn_amd as pkg
    scs = []
    for _ in range(2):
        sc = pkg.Scorer(0)
        sc.set_builtin_networks(5)
        scs.append(sc)
    yield tuple(scs)
    for sc in scs:
        sc.close()


def same_round(a, b, what=None):
    for f in ARRAYS:
        assert a[f].dtype == b[f].dtype and np.array_equal(a[f], b[f]), (what, f)
    assert (a["n_total"], a["new_strat"], a["counters"]) == (b["n_total"], b["new_strat"], b["counters"]), what


# ------------------------------------------------------------------------------------------ 1. tables
@pytest.mark.parametrize("case", ["spar020", "mixed"])
def test_tables_equal_the_twin_bit_for_bit(scorers, case):
    from sdpcutsel_via_nn_amd import nodebox
    sc, _ = scorers
    n, Q, S, ks = bind(sc, case)
    assert sc.box is None
    lb, ub = nc.random_box(n, 11)
    sc.set_box(lb, ub)
    got = sc.box
    assert np.array_equal(got[0], lb) and np.array_equal(got[1], ub)
    Qb, none = sc.box_tables(point=False)
    assert none is None and np.array_equal(Qb.view(np.uint64), nodebox.transform_tables(Q, None, lb, ub)[0].view(np.uint64))
    for seed, outside in ((11, False), (12, True)):      # a first and a second set_point
        vv = nc.point_in_box(n, lb, ub, seed, outside=outside)
        sc.set_point(vv)
        Qb, vb = sc.box_tables()
        tQ, tv = nodebox.transform_tables(Q, vv, lb, ub)
        assert np.array_equal(Qb.view(np.uint64), tQ.view(np.uint64)) and np.array_equal(vb.view(np.uint64), tv.view(np.uint64))
    # set_box on a handle that has a point already: both tables follow
    lb2, ub2 = nc.random_box(n, 13)
    sc.set_box(lb2, ub2)
    Qb, vb = sc.box_tables()
    tQ, tv = nodebox.transform_tables(Q, vv, lb2, ub2)
    assert np.array_equal(Qb.view(np.uint64), tQ.view(np.uint64)) and np.array_equal(vb.view(np.uint64), tv.view(np.uint64))
    # the unit box: the originals' bits
    sc.set_box(np.zeros(n), np.ones(n))
    Qb, vb = sc.box_tables()
    assert np.array_equal(Qb, Q) and np.array_equal(vb, vv)
    sc.clear_box()
    assert sc.box is None


# ------------------------------------------------------------------------------------------ 2. unit box = no box
@pytest.mark.parametrize("case", ["spar020", "mixed"])
def test_unit_box_and_cleared_box_equal_no_box(scorers, case):
    from sdpcutsel_via_nn_amd import harness
    sc, plain = scorers
    n, Q, S, ks = bind(sc, case)
    bind(plain, case)
    vv = harness.random_mccormick_point(n, np.random.default_rng(21))
    N = S.shape[0]

    def compare(tag):
        for h in (sc, plain):
            h.set_point(vv)
            h.score(EIG | NN)
        a, b = sc.get_scores(), plain.get_scores()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), tag
        for strat in (1, 2, 4):
            for sel in (64, N):
                same_round(sc.round_csr(strat, sel, point=vv, copy=True), plain.round_csr(strat, sel, point=vv, copy=True), (tag, strat, sel))

    sc.set_box(np.zeros(n), np.ones(n))
    compare("unit box")
    sc.set_box(*nc.random_box(n, 22))
    sc.set_point(vv)
    sc.score(NN)
    assert not np.array_equal(sc.get_scores(eig=False)[1], plain.get_scores(eig=False)[1])      # (the box does change the measure)
    sc.clear_box()
    compare("cleared box")


# ------------------------------------------------------------------------------------------ 3. re-expression, exact
@pytest.mark.parametrize("case", ["mixed", "spar020"])
def test_reexpressed_instance_scores_identically(scorers, case):
    """Instance A lives on the unit box (integer Q_A, a point on the 2^-20 grid); instance B is the same problem in the stretched
    variables y = l + D x, d_i in {1, 1/2, 1/4, 1/8}, l_i on the 2^-6 grid.  Every product of the map fits 53 bits (asserted with
    fractions), so B's tables under the box [l, l + d] ARE A's tables and B's measure is A's, bit for bit."""
    from sdpcutsel_via_nn_amd import harness, nodebox
    sc, plain = scorers
    inst, S, ks = _COVERS[case] if case in _COVERS else _COVERS.setdefault(case, cover(case))
    n = inst["nb_vars"]
    L = n * (n + 1) // 2
    rng = np.random.default_rng(31)
    QA = np.rint(2.0 * np.asarray(inst["Q_arr"], dtype=np.float64))
    assert np.array_equal(QA, np.rint(QA)) and np.abs(QA).max() >= 2
    vA = np.rint(harness.random_mccormick_point(n, rng) * 2.0 ** 20) / 2.0 ** 20
    d = 2.0 ** -rng.integers(0, 4, n).astype(np.float64)
    l = np.floor(rng.uniform(0.0, 1.0, n) * (1.0 - d) * 64.0) / 64.0
    assert set(d.tolist()) == {1.0, 0.5, 0.25, 0.125} and np.all(l + d <= 1.0) and np.all(l >= 0)
    i, j = np.triu_indices(n)
    QB = QA / (d[i] * d[j])
    y = l + d * vA[L:]
    YB = ((d[i] * d[j]) * vA[:L] + l[i] * y[j]) + l[j] * y[i] - l[i] * l[j]
    vB = np.concatenate([YB, y])
    # exactness with fractions: the construction, and the device's map in its own operation order
    F = Fraction
    fl, fd, fx, fX, fQ = [F(v) for v in l], [F(v) for v in d], [F(v) for v in vA[L:]], [F(v) for v in vA[:L]], [F(v) for v in QA]
    fy = [fl[a] + fd[a] * fx[a] for a in range(n)]
    assert all(F(float(v)) == v for v in fy) and all(F(y[a]) == fy[a] for a in range(n))
    for p in range(L):
        a, b = int(i[p]), int(j[p])
        t = fd[a] * fd[b] * fX[p] + fl[a] * fy[b] + fl[b] * fy[a] - fl[a] * fl[b]
        assert F(YB[p]) == t and F(QB[p]) == fQ[p] / (fd[a] * fd[b])
        steps = [fl[a] * fy[b], t - fl[a] * fy[b], fl[b] * fy[a], t - fl[a] * fy[b] - fl[b] * fy[a], fl[a] * fl[b], fd[a] * fd[b] * fX[p], fd[a] * fd[b]]
        assert all(F(float(s)) == s for s in steps)      # every intermediate of box.hip is a double
    tQ, tv = nodebox.transform_tables(QB, vB, l, l + d)
    assert np.array_equal(tQ, QA) and np.array_equal(tv, vA)
    # A plain, B boxed
    plain.drop_pending()
    plain.set_instance(n, QA)
    plain.set_candidates(S, ks)
    plain.set_point(vA)
    plain.score(NN)
    sc.drop_pending()
    sc.set_instance(n, QB)
    sc.set_candidates(S, ks)
    sc.set_box(l, l + d)
    sc.set_point(vB)
    sc.score(NN)
    Qb, vb = sc.box_tables()
    assert np.array_equal(Qb, QA) and np.array_equal(vb, vA)
    objA, objB = plain.get_scores(eig=False)[1], sc.get_scores(eig=False)[1]
    assert np.array_equal(objB, objA) and np.abs(objA).max() > 0
    sc.clear_box()


# ------------------------------------------------------------------------------------------ 4. composition
def _composition(sc, plain, case, seed, outside):
    from sdpcutsel_via_nn_amd import nodebox
    n, Q, S, ks = bind(sc, case)
    lb, ub = nc.random_box(n, seed)
    vv = nc.point_in_box(n, lb, ub, seed, outside=outside)
    tQ, tv = nodebox.transform_tables(Q, vv, lb, ub)
    sc.set_box(lb, ub)
    sc.set_point(vv)
    sc.score(EIG | NN)
    eig, obj = sc.get_scores()
    bind(plain, case, Q=tQ)
    plain.set_point(tv)
    plain.score(NN)
    assert np.array_equal(obj, plain.get_scores(eig=False)[1])
    bind(plain, case)
    plain.set_point(vv)
    plain.score(EIG | NN)
    e0, o0 = plain.get_scores()
    assert np.array_equal(eig, e0) and not np.array_equal(obj, o0)
    sc.clear_box()


@pytest.mark.parametrize("variant", [0, 2, 1])      # MFMA, VALU, simple
@pytest.mark.parametrize("case,seed,outside", [("spar020", 41, False), ("mixed", 42, True)])
def test_boxed_scores_compose(scorers, case, seed, outside, variant):
    from sdpcutsel_via_nn_amd import _capi
    sc, plain = scorers
    try:
        for h in scorers:
            h.set_option(_capi.OPT_KERNEL, variant)
        _composition(sc, plain, case, seed, outside)
    finally:
        for h in scorers:
            h.set_option(_capi.OPT_KERNEL, _capi.KERNEL_MFMA)


def test_boxed_scores_compose_on_a_user_network():
    import sdpcutsel_via_nn_amd as pkg
    import user_nets
    scs = [pkg.Scorer(0), pkg.Scorer(0)]
    try:
        for h in scs:
            for k in (2, 3, 4, 5):
                h.set_network(k, *user_nets.shaped_network(k, 38.5))
        _composition(scs[0], scs[1], "mixed", 43, False)
    finally:
        for h in scs:
            h.close()


# ------------------------------------------------------------------------------------------ 5. rounds
def ranking(strat, obj, lam, sel):
    """the reference's ranking (cut_select_qp.py:601-632) restated: -> (order, score in order, new_strat, strong, violated)"""
    N = obj.shape[0]
    sel = min(sel, N)
    first = np.argsort(-obj, kind="stable")
    if strat == 2:
        return first, obj[first], 2, None, None
    s = obj[first]
    viol = lam[first] < -1e-15
    pos = s > 0
    strong = pos & viol
    visited = (np.cumsum(strong) - strong) < sel
    new = s.copy()
    up, down, low = visited & strong, visited & pos & ~viol, visited & ~pos & viol
    new[up] = s[up] + 1000.0
    new[down] = s[down] - 1000.0
    new[low] = -lam[first][low]
    second = np.argsort(-new, kind="stable")
    n_strong, n_viol = int(up.sum()), int(up.sum()) + int(low.sum())
    return first[second], new[second], (1 if sel > 0 and n_strong / sel < n_viol / N else 4), n_strong, n_viol


@pytest.mark.parametrize("strat", [2, 4])
@pytest.mark.parametrize("case,seed", [("spar020", 51), ("mixed", 52)])
def test_boxed_round_ranks_its_own_scores_and_cuts_at_the_original_point(scorers, case, seed, strat):
    sc, plain = scorers
    n, Q, S, ks = bind(sc, case)
    bind(plain, case)
    lb, ub = nc.random_box(n, seed)
    vv = nc.point_in_box(n, lb, ub, seed, outside=True)
    sc.set_box(lb, ub)
    plain.set_point(vv)
    if strat == 4:
        plain.score(EIG)      # (as in a plain combined round: the row assembly starts from a scored lambda_min where there is one)
    N = S.shape[0]
    for sel in (37, 100, N):
        r = sc.round_csr(strat, sel, point=vv, copy=True)
        sc.score(EIG | NN)      # (whatever the round left unscored)
        eig, obj = sc.get_scores()
        order, score, new_strat, n_strong, n_viol = ranking(strat, obj, eig, sel)
        w = min(sel, N)
        assert r["idx"].shape[0] == w and np.array_equal(r["idx"], order[:w]) and np.array_equal(r["score"], score[:w]), (sel,)
        assert r["new_strat"] == new_strat and r["n_total"] == N
        if strat == 4:
            assert r["counters"]["strong"] == n_strong and r["counters"]["violated"] == n_viol
        else:
            assert r["counters"]["nb_positive"] == int(np.count_nonzero(obj > 0))
        # the rows: those of a plain handle for the same ids at the ORIGINAL point
        lam, coef, rhs, cols, kk = plain.cut_rows(r["idx"])
        assert np.array_equal(r["lam"], lam) and np.array_equal(r["ks"], kk)
        ent = np.flatnonzero(lam < -1e-15)
        assert ent.size > 0 and np.array_equal(r["row_entry"], ent) and np.array_equal(r["rhs"], rhs[ent])
        for row, e in enumerate(ent):
            lo, hi = r["indptr"][row], r["indptr"][row + 1]
            assert np.array_equal(r["values"][lo:hi], coef[e, :hi - lo]) and np.array_equal(r["indices"][lo:hi], cols[e, :hi - lo])
    sc.clear_box()


def test_diverse_multi_and_pool_rounds_run_on_a_boxed_handle(scorers):
    from sdpcutsel_via_nn_amd import cutpool, diversity, multicut
    sc, plain = scorers
    n, Q, S, ks = bind(sc, "spar020")
    lb, ub = nc.random_box(n, 61)
    vv = nc.point_in_box(n, lb, ub, 61)
    sc.set_box(lb, ub)
    N = S.shape[0]
    for strat in (2, 4):
        quota, mp, pool = 60, 0.5, 257
        sc.set_point(vv)
        sc.score(EIG | NN)
        ids, score, total, _, _ = sc.rank(strat, quota, max_out=N)
        P = min(pool, ids.shape[0])
        lam, coef, _, _, kk = sc.cut_rows(ids[:P])
        el = diversity.eligible_rows(lam, ks[ids[:P]], coef)
        r = sc.round_csr_diverse(None, strat, quota, mp, pool_size=pool, copy=True)
        pos = {int(g): t for t, g in enumerate(ids[:P])}
        keep = np.zeros(P, dtype=bool)
        keep[[pos[int(g)] for g in r["idx"]]] = True
        assert keep.sum() == r["idx"].shape[0] > 0 and np.array_equal(ids[:P][keep], r["idx"])
        assert diversity.check_walk(S[ids[:P]], ks[ids[:P]], coef, el, quota, mp, keep, margin=1e-12, examined=r["info"]["examined"])
        # multi-cut round: the head of the plain boxed round, rows by the checker at the original point
        m, cap = 3, 100
        head = sc.round_csr(strat, cap, point=vv, copy=True)
        res = sc.round_csr_multi(vv, strat, cap, m, row_quota="sets", copy=True)
        assert np.array_equal(res["idx"], head["idx"]) and np.array_equal(res["score"], head["score"])
        rows = res["rhs"].shape[0]
        assert rows > 0
        cf = np.zeros((rows, 20))
        for t in range(rows):
            lo, hi = res["indptr"][t], res["indptr"][t + 1]
            cf[t, :hi - lo] = res["values"][lo:hi]
        idx = res["idx"]
        assert multicut.check_rows(S[idx], ks[idx], vv, n, m, res["row_entry"], res["row_rank"], res["row_lam"], cf, res["rhs"], row_quota=m * cap)
    # a pool step: the rows of a boxed round, stepped at a second point of the node
    head = sc.round_csr(4, 100, point=vv, copy=True)
    sc.pool_create(512)
    sc.pool_add(head["indptr"], head["indices"], head["values"], head["rhs"])
    par = dict(tight_tol=1e-9, viol_tol=1e-6, max_age=1, drop_age=2, max_return=8)
    for seed in (62, 63):
        v2 = nc.point_in_box(n, lb, ub, seed)
        before = sc.pool_state()
        out = sc.pool_step(v2, **par)
        assert cutpool.check_step(before, par, v2, out, sc.pool_state())
    r2 = sc.round_csr(4, 100, copy=True)      # the round behind the step, at the step's point
    sc.pool_destroy()
    sc.set_point(v2)
    same_round(r2, sc.round_csr(4, 100, copy=True))
    sc.clear_box()


# ------------------------------------------------------------------------------------------ 6. unaffected strategies
@pytest.mark.parametrize("case", ["spar020", "mixed"])
def test_strategies_without_a_measure_ignore_the_box(scorers, case):
    sc, plain = scorers
    n, Q, S, ks = bind(sc, case)
    bind(plain, case)
    lb, ub = nc.random_box(n, 71)
    vv = nc.point_in_box(n, lb, ub, 71)
    sc.set_box(lb, ub)
    # strategy 1: the feasibility round; strategy 0: the dense eigen-cuts; strategy 5 (random order): its rows are cut_rows'
    same_round(sc.round_csr(1, 100, point=vv, copy=True), plain.round_csr(1, 100, point=vv, copy=True), "feasibility")
    a, b = sc.dense_round(vv), plain.dense_round(vv)
    assert a["n_rows"] == b["n_rows"] and np.array_equal(a["values"], b["values"]) and np.array_equal(a["rhs"], b["rhs"])
    ids = np.random.default_rng(71).permutation(S.shape[0])[:200]
    sc.set_point(vv)
    plain.set_point(vv)
    for x, y in zip(sc.cut_rows(ids), plain.cut_rows(ids)):
        assert np.array_equal(x, y)
    sc.clear_box()


# ------------------------------------------------------------------------------------------ 7. exact measure
def _sdp_inputs(k, S_k, Q, vv, n):
    """[x | Q_slice], max_elem and (-S) max_elem of the size-k candidates as gather.h forms them"""
    L = n * (n + 1) // 2
    rows, me, neg = [], [], []
    for s in S_k:
        pos = [n * int(s[a]) - int(s[a]) * (int(s[a]) + 1) // 2 + int(s[b]) for a in range(k) for b in range(a, k)]
        q = Q[pos]
        m = float(k) * float(np.abs(q).max())
        m = m if m != 0.0 else 1.0
        qs = q / m
        acc = 0.0
        for t, p in enumerate(pos):
            acc = acc + qs[t] * vv[p]
        rows.append(np.concatenate([vv[L + s[:k]], qs]))
        me.append(m)
        neg.append((-acc) * m)
    return np.array(rows), np.array(me), np.array(neg)


@pytest.mark.parametrize("case,seed", [("spar020", 81), ("mixed", 82)])
def test_exact_measure_on_a_boxed_handle(case, seed):
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import _capi, nodebox
    scs = [pkg.Scorer(0), pkg.Scorer(0)]
    try:
        sc, plain = scs
        for h in scs:
            h.set_option(_capi.OPT_EXACT_SDP, 1)
        n, Q, S, ks = bind(sc, case)
        lb, ub = nc.random_box(n, seed)
        vv = nc.point_in_box(n, lb, ub, seed, outside=True)
        tQ, tv = nodebox.transform_tables(Q, vv, lb, ub)
        sc.set_box(lb, ub)
        sc.set_point(vv)
        sc.score(SDP)
        val, gap = sc.get_sdp_scores()
        unconv = sc.get_stat(_capi.STAT_SDP_UNCONVERGED)
        bind(plain, case, Q=tQ)
        plain.set_point(tv)
        plain.score(SDP)
        pv, pg = plain.get_sdp_scores()
        assert np.array_equal(val, pv) and np.array_equal(gap, pg) and unconv == plain.get_stat(_capi.STAT_SDP_UNCONVERGED)
        # a lower bound within the certificate's gap M' of the solver on the twin-transformed inputs
        for k in sorted(set(ks.tolist())):
            sel = np.flatnonzero(ks == k)
            inp, me, neg = _sdp_inputs(k, S[sel], tQ, tv, n)
            bv, bg = plain.sdp_batch(k, inp)
            lower, upper = neg + bv * me, neg + (bv + bg) * me
            tiny = 8 * 2.0 ** -53 * (np.abs(neg) + np.abs(bv * me) + bg * me)
            assert np.all(val[sel] <= upper + tiny) and np.all(val[sel] >= lower - gap[sel] * me - tiny)
            assert np.all(gap[sel] >= 0)
        # strategy 3 ranks that measure
        r = sc.round_csr(3, 50, copy=True)
        order = np.argsort(-val, kind="stable")[:50]
        assert np.array_equal(r["idx"], order) and np.array_equal(r["score"], val[order]) and r["new_strat"] == 3
    finally:
        for h in scs:
            h.close()


# ------------------------------------------------------------------------------------------ 8. state and refusals
def test_state_and_refusals(scorers):
    import torch
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import _capi
    sc, plain = scorers
    n, Q, S, ks = bind(sc, "spar020")
    lb, ub = nc.random_box(n, 91)
    vv = nc.point_in_box(n, lb, ub, 91)
    sc.set_point(vv)
    sc.score(EIG | NN)
    e0, o0 = sc.get_scores()
    assert sc.get_stat(_capi.STAT_SCORED) == (EIG | NN)
    # set_box after scoring: the measure is gone, lambda_min stays
    sc.set_box(lb, ub)
    assert sc.get_stat(_capi.STAT_SCORED) == EIG
    assert np.array_equal(sc.get_scores(obj=False)[0], e0)
    with pytest.raises(pkg.SdpCutError, match="not scored"):
        sc.get_scores(eig=False)
    sc.score(NN)
    e1, o1 = sc.get_scores()
    assert np.array_equal(e1, e0) and not np.array_equal(o1, o0)
    # bad boxes: refused by the library itself (the binding's own check is bypassed), the box in place stays
    import ctypes
    dp = ctypes.POINTER(ctypes.c_double)
    for i_lb, i_ub in ((-1e-12, 1.0), (0.0, 1.0 + 1e-12), (float("nan"), 1.0), (0.0, float("inf")), (0.5, 0.5), (0.5, 0.5 + 2.0 ** -11)):
        l2, u2 = np.zeros(n), np.ones(n)
        l2[3], u2[3] = i_lb, i_ub
        assert sc._lib.sdpcut_set_box(sc._h, l2.ctypes.data_as(dp), u2.ctypes.data_as(dp)) == -1
        assert "set_box" in sc._lib.sdpcut_last_error(sc._h).decode()
    assert sc._lib.sdpcut_set_box(sc._h, lb.ctypes.data_as(dp), None) == -1
    assert np.array_equal(sc.box[0], lb) and sc.get_stat(_capi.STAT_SCORED) == (EIG | NN)
    # the refused calls leave box, point and scores alone: the round behind them is the round before them
    sel = 100
    before = sc.round_csr(4, sel, point=vv, copy=True)
    pts = np.stack([vv, vv])
    rec = torch.zeros(8 + 3 * 64, dtype=torch.int64, device="cuda")
    refused = [lambda: sc.score_points(pts), lambda: sc.round_csr_points(pts, 4, sel),
               lambda: sc.shard_head_device(_capi.STRAT_OPT, 64, rec.data_ptr()),
               lambda: sc.shard_finish_enqueue(1, 64, rec.data_ptr(), 32),
               lambda: sc.shard_finish_round(1, 64, rec.data_ptr(), 32),
               lambda: sc.set_option(_capi.OPT_EXACT_HEAD, 1)]
    for call in refused:
        with pytest.raises(pkg.SdpCutError, match="node box"):
            call()
        assert np.array_equal(sc.box[0], lb) and np.array_equal(sc.box[1], ub) and sc.get_stat(_capi.STAT_SCORED) == (EIG | NN)
        same_round(sc.round_csr(4, sel, copy=True), before)
    e2, o2 = sc.get_scores()
    assert np.array_equal(e2, e1) and np.array_equal(o2, o1)
    # ... and a handle with SDPCUT_OPT_EXACT_HEAD on refuses a box
    bind(plain, "spar020")
    plain.set_option(_capi.OPT_EXACT_HEAD, 1)
    try:
        with pytest.raises(pkg.SdpCutError, match="EXACT_HEAD"):
            plain.set_box(lb, ub)
        assert plain.box is None
    finally:
        plain.set_option(_capi.OPT_EXACT_HEAD, 0)
    # set_instance clears the box
    sc.set_instance(n, Q)
    assert sc.box is None
    with pytest.raises(pkg.SdpCutError, match="no node box"):
        sc.box_tables()


# ------------------------------------------------------------------------------------------ 9. / 10. the solver classes
def _solver(case):
    import sdpcutsel_via_nn_amd as pkg
    inst, S, ks = _COVERS[case] if case in _COVERS else _COVERS.setdefault(case, cover(case))
    n = inst["nb_vars"]
    cs = pkg.CutSolver()
    sets = [[int(v) for v in S[t, :ks[t]]] for t in range(S.shape[0])]
    agg = [(s, [n * s[a] - s[a] * (s[a] + 1) // 2 + s[b] for a in range(len(s)) for b in range(a, len(s))], None, None) for s in sets]
    cs.set_instance(n, np.asarray(inst["Q_arr"], dtype=np.float64), agg, dim=3)
    return cs, n


def test_separate_points_with_boxes(scorers):
    sc, _ = scorers
    cs, n = _solver("spar020")
    bind(sc, "spar020")
    boxes = np.stack([np.stack(nc.random_box(n, 100 + p)) for p in range(3)])
    pts = np.stack([nc.point_in_box(n, boxes[p, 0], boxes[p, 1], 100 + p) for p in range(3)])
    for strat in (2, 4):
        nodes = cs.separate_points(strat, pts, 100, boxes=boxes)
        assert len(nodes) == 3
        for p, (csr, n_total, new_strat, counters) in enumerate(nodes):
            sc.set_box(boxes[p, 0], boxes[p, 1])
            ref = sc.round_csr(strat, 100, point=pts[p], copy=True)
            assert (n_total, new_strat, counters) == (ref["n_total"], ref["new_strat"], ref["counters"])
            for got, f in zip(csr, ("indptr", "indices", "values", "rhs")):
                assert np.array_equal(got, ref[f]), (strat, p, f)
    with pytest.raises(ValueError):
        cs.separate_points(2, pts, 100, boxes=boxes[:2])
    # the solver is back at the root: the batched call without boxes is served again
    assert len(cs.separate_points(2, pts, 100)) == 3
    sc.clear_box()


def test_set_node_box_reaches_bound_and_later_handles(scorers):
    sc, plain = scorers
    cs, n = _solver("spar020")
    n, Q, S, ks = bind(sc, "spar020")
    bind(plain, "spar020")
    lb, ub = nc.random_box(n, 111)
    vv = nc.point_in_box(n, lb, ub, 111)
    sc.set_box(lb, ub)

    def head(solver, strat):
        r = solver._sel_eigcut_by_ordering_on_measure(strat, vv, 1, **({"sel_size": 100} if strat == 4 else {}))
        rl = r[1] if isinstance(r, tuple) else r
        return rl.ids(100).copy(), rl.scores(100).copy()

    def ref(h, strat):
        r = h.round_csr(strat, 100, point=vv, copy=True)
        return r["idx"], r["score"]

    def same(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])

    for strat in (2, 4):
        assert same(head(cs, strat), ref(plain, strat))          # the list is bound now, at the root
        cs.set_node_box(lb, ub)
        boxed = head(cs, strat)
        assert same(boxed, ref(sc, strat)) and not same(boxed, ref(plain, strat))
        cs.set_node_box(None, None)
        assert same(head(cs, strat), ref(plain, strat))
    # a handle the solver creates after the call: a host-side list through _gpu_bind, arrays through gpu_bind_arrays
    cs2, _ = _solver("spar020")
    cs2.set_node_box(lb, ub)
    assert same(head(cs2, 2), ref(sc, 2))
    b = cs2.gpu_bind_arrays(S, ks, n, Q)
    assert np.array_equal(b.scorer.box[0], lb) and np.array_equal(b.scorer.box[1], ub)
    cs2.set_node_box(0.0, 1.0)                                   # scalars are broadcast; the unit box is a box
    assert same(head(cs2, 2), ref(plain, 2))
    with pytest.raises(ValueError):
        cs2.set_node_box(0.5, 0.5)
    sc.clear_box()


def test_cut_select_algo_at_a_node(scorers):
    import os
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import harness
    sc, _ = scorers
    inst, _ = nc.instance("spar020")
    path = os.path.join(nc.INST, nc.CASES["spar020"][0])
    lb, ub, root = nc.child_box(inst, 1)
    n = inst["nb_vars"]
    cs = pkg.CutSolver()
    out = cs.cut_select_algo(path, 3, 0.1, strat=2, nb_rounds_cuts=2, box=(lb, ub))
    bounds, cuts, n_cand = out[0], out[4], out[6]
    assert len(bounds) == 3 and n_cand == 1051
    # the function reports -LP value of a minimisation: the LP value does not decrease from round to round
    lp_vals = [-b for b in bounds]
    assert lp_vals[0] >= root - 1e-7 * abs(root) and lp_vals[1] >= lp_vals[0] - 1e-9 * abs(lp_vals[0]) and lp_vals[2] >= lp_vals[1] - 1e-9 * abs(lp_vals[1])
    # round 1: the cuts of a boxed round at the node's LP point (one row per violated head entry)
    lp = harness.boxqp_relaxation(inst, lb, ub)
    lp.solve()
    bind(sc, "spar020")
    sc.set_box(lb, ub)
    quota = pkg.CutSolver.selection_size(0.1, n_cand)
    r = sc.round_csr(2, quota, point=np.asarray(lp.get_values(), dtype=np.float64), copy=True)
    assert r["idx"].shape[0] == quota and cuts[1] == r["rhs"].shape[0] and 0 < cuts[1] <= quota
    sc.clear_box()
    # box=None and the unit box: the same run
    a = cs.cut_select_algo(path, 3, 0.1, strat=2, nb_rounds_cuts=2)
    b = cs.cut_select_algo(path, 3, 0.1, strat=2, nb_rounds_cuts=2, box=(0.0, 1.0))
    assert a[0] == b[0] and a[4] == b[4] and a[5] == b[5] and a[6] == b[6]      # (the other entries are wall-clock times)
    with pytest.raises(ValueError):
        cs.cut_select_algo(path, 3, 0.1, strat=2, nb_rounds_cuts=1, box=(0.5, 0.5))
