"""Diverse cut selection on the device (sdpcut_round_csr_diverse, sdpcut_filter_parallel; csrc/diverse.hip) against the numpy twin
of the walk (sdpcutsel_via_nn_amd/diversity.py), which runs on rows fetched with Scorer.cut_rows.

Where the comparison is exact (test 2) the test FIRST asserts that no pair of the pool has a cosine within 1e-12 of the threshold
and that neighbouring ranking scores inside the pool differ by more than 1e-12: the device's products may differ from numpy's in
the last bit, and only a pair that close could be decided differently.  At the structured vertex (test 3) cosines tie exactly, so
the device's answer is checked against the invariants of the walk instead (diversity.check_walk)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INST = os.path.join(ROOT, "tests", "golden", "instances")
ARRAYS = ("idx", "score", "lam", "ks", "set_inds", "row_entry", "indptr", "indices", "values", "rhs")
MARGIN = 1e-12


@pytest.fixture(scope="module")
def scorers():
    """two handles with the four shipped networks: the one under test and a fresh one to compare with"""
    import sdpcutsel_via_nn_amd as pkg
    scs = []
    for _ in range(2):
        sc = pkg.Scorer(0)
        sc.set_builtin_networks(5)
        scs.append(sc)
    yield tuple(scs)
    for sc in scs:
        sc.close()


def boxqp_cover(name, dim):
    from sdpcutsel_via_nn_amd import _capi, harness
    inst = harness.parse_boxqp(os.path.join(INST, name))
    S, ks, _ = _capi.enumerate_cover(inst["adj"], dim)
    return inst, np.ascontiguousarray(S), np.ascontiguousarray(ks)


def bind(sc, case):
    """-> (n, set_inds [N, 5], ks [N]) of the list now on the handle"""
    from sdpcutsel_via_nn_amd import synthetic
    sc.drop_pending()
    if case == "philox":      # 1000 three-variable candidates on n = 200: variable indices pass 128
        n = 200
        Q_arr, _, _ = synthetic.make_instance(n, 7)
        sc.set_instance(n, np.asarray(Q_arr, dtype=np.float64))
        sc.set_candidates_philox(3, 1000, seed=7)
        S, ks = sc.get_candidates(np.arange(1000))
        return n, S, ks
    inst, S, ks = boxqp_cover(*{"spar020": ("spar020-100-1.in", 3), "mixed": ("spar040-030-1.in", 5)}[case])
    sc.set_instance(inst["nb_vars"], np.asarray(inst["Q_arr"], dtype=np.float64))
    sc.set_candidates(S, ks)
    return inst["nb_vars"], S, ks


def random_point(n, seed):
    from sdpcutsel_via_nn_amd import harness
    return harness.random_mccormick_point(n, np.random.default_rng(seed))


def mccormick_vertex(inst):
    """the optimum of the McCormick relaxation of a BoxQP instance: x = 0.5, X_ii = 0.5, X_ij in {0, 0.5} by the sign of q_ij"""
    n = inst["nb_vars"]
    Q = np.asarray(inst["Q_arr"], dtype=np.float64)
    X = np.where(Q < 0, 0.5, 0.0)
    iu = np.triu_indices(n)
    X[iu[0] == iu[1]] = 0.5
    return np.concatenate([X, np.full(n, 0.5)])


def pool_rows(sc, S, ks, local_ids):
    """what the twin needs of the pool: index sets, sizes, rows, eligibility (rows from the device, at the current point)"""
    from sdpcutsel_via_nn_amd import diversity
    lam, coef, _, _, kk = sc.cut_rows(local_ids)
    assert np.array_equal(kk, ks[local_ids])
    return S[local_ids], ks[local_ids], coef, diversity.eligible_rows(lam, ks[local_ids], coef)


FLAGS = {1: 1, 2: 2, 4: 3}


# ------------------------------------------------------------------------------------------ 1. rows
@pytest.mark.parametrize("seed", [7, 8])
def test_filter_without_comparison_keeps_the_first_eligible(scorers, seed):
    sc, _ = scorers
    n, S, ks = bind(sc, "spar020")
    sc.set_point(random_point(n, seed))
    rng = np.random.default_rng(seed)
    order = rng.permutation(S.shape[0])[:700]
    order[350] = order[3]       # a caller's list may hold a candidate twice
    Sp, kp, coef, el = pool_rows(sc, S, ks, order)
    assert 0 < el.sum() < 700 or el.all()
    for quota in (1, 64, 100, 700):
        keep, info = sc.filter_parallel(order, quota, 1.0)
        want = np.zeros(700, dtype=bool)
        want[np.flatnonzero(el)[:quota]] = True
        assert np.array_equal(keep, want), quota
        examined = int(np.flatnonzero(want)[-1]) + 1 if want.sum() >= quota else 700
        assert info == dict(pool=700, examined=examined, skipped_nonviolated=int((~el[:examined]).sum()), rejected_parallel=0)


@pytest.mark.parametrize("strat", [1, 2, 4])
@pytest.mark.parametrize("seed", [7, 8])
def test_no_filter_equals_the_plain_round(scorers, strat, seed):
    """max_parallel = 1, pool = sel: every head array and CSR array of the plain round restricted to its cut-yielding entries"""
    sc, _ = scorers
    n, S, ks = bind(sc, "spar020")
    vv = random_point(n, seed)
    for sel in (100, 105, S.shape[0]):
        a = sc.round_csr(strat, sel, point=vv, copy=True)
        d = sc.round_csr_diverse(vv, strat, sel, 1.0, pool_size=sel, copy=True)
        e = a["row_entry"]
        assert e.shape[0] > 0
        for f in ("idx", "score", "lam", "ks", "set_inds"):
            assert d[f].dtype == a[f].dtype and np.array_equal(d[f], a[f][e]), (sel, f)
        for f in ("indptr", "indices", "values", "rhs"):
            assert d[f].dtype == a[f].dtype and np.array_equal(d[f], a[f]), (sel, f)
        assert np.array_equal(d["row_entry"], np.arange(e.shape[0], dtype=np.int32))
        assert (d["n_total"], d["new_strat"], d["counters"]) == (a["n_total"], a["new_strat"], a["counters"])
        w = a["idx"].shape[0]
        assert d["info"] == dict(pool=w, examined=w, skipped_nonviolated=w - e.shape[0], rejected_parallel=0)


# ------------------------------------------------------------------------------------------ 2. the walk, exactly
CASES = [("spar020", 7, 1), ("spar020", 7, 2), ("spar020", 7, 4), ("spar020", 8, 1), ("spar020", 8, 2), ("spar020", 8, 4),
         ("mixed", 7, 1), ("mixed", 7, 4), ("philox", 7, 1), ("philox", 7, 2)]


@pytest.mark.parametrize("case,seed,strat", CASES)
def test_walk_equals_the_twin(scorers, case, seed, strat):
    from sdpcutsel_via_nn_amd import diversity
    sc, _ = scorers
    n, S, ks = bind(sc, case)
    sc.set_point(random_point(n, seed))
    sc.score(FLAGS[strat])
    full = S.shape[0]
    checked = 0
    for quota in (1, 37, 100):
        pools = sorted(set(p for p in (quota, 63, 64, 65, 257, full) if quota <= p <= full))
        # the ranking depends on the quota under the combined strategy only; one pair matrix per ranking serves all its prefixes
        ids, score, total, _, _ = sc.rank(strat, quota, max_out=full)
        loc = ids - sc.base
        Sp, kp, coef, el = pool_rows(sc, S, ks, loc)
        dots = diversity.pair_dots(Sp, kp, coef)
        den = dots[1][:, None] * dots[1][None, :]
        cos = np.divide(dots[0], den, out=np.zeros_like(dots[0]), where=den > 0)
        gaps = np.abs(np.diff(score))
        print("%s seed %d strat %d quota %d: ranking of %d, min score gap %.3e, eligible %d" % (case, seed, strat, quota, ids.shape[0],
                                                                                             gaps.min() if gaps.size else np.inf, el.sum()))
        assert gaps.size == 0 or gaps.min() > MARGIN
        for mp in (0.1, 0.5, 0.9):
            near = np.abs(np.abs(cos[np.tril_indices(cos.shape[0], -1)]) - mp)
            print("    max_parallel %.1f: closest |cos| to the threshold %.3e away" % (mp, near.min()))
            assert diversity.undecided_pairs(Sp, kp, coef, el, mp, MARGIN, cos=cos).shape[0] == 0
            for pool in pools:
                P = min(pool, ids.shape[0])
                keep_t, info_t = diversity.greedy_filter(Sp[:P], kp[:P], coef[:P], el[:P], quota, mp, return_info=True, dots=dots)
                assert info_t.pop("closest") > MARGIN
                keep_d, info_d = sc.filter_parallel(loc[:P], quota, mp)
                assert np.array_equal(keep_d, keep_t), (quota, mp, pool)
                assert info_d == info_t, (quota, mp, pool)
                r = sc.round_csr_diverse(None, strat, quota, mp, pool_size=pool)
                assert np.array_equal(r["idx"], ids[:P][keep_t]), (quota, mp, pool)
                assert np.array_equal(r["score"], score[:P][keep_t])
                assert r["info"] == info_t, (quota, mp, pool)
                assert r["rhs"].shape[0] == r["idx"].shape[0] and np.array_equal(r["row_entry"], np.arange(r["idx"].shape[0]))
                assert r["n_total"] == total
                checked += 1
    assert checked >= 9


def test_largest_pool(scorers):
    """16384 entries, the most a call takes: every block of the bit matrix, every word of the accepted mask.  The twin computes only
    the columns of accepted entries; `closest` is the distance from the threshold of the nearest pair the outcome depends on.
    The list is drawn with replacement from 9880 triples: it holds candidates twice (cos = 1)."""
    from sdpcutsel_via_nn_amd import _capi, diversity, synthetic
    sc, _ = scorers
    sc.drop_pending()
    n, N = 40, _capi.DIVERSE_MAX_POOL
    Q_arr, _, _ = synthetic.make_instance(n, 7)
    sc.set_instance(n, np.asarray(Q_arr, dtype=np.float64))
    sc.set_candidates_philox(3, N, seed=11)
    S, ks = sc.get_candidates(np.arange(N))
    assert np.unique(S[:, :3], axis=0).shape[0] < N
    sc.set_point(random_point(n, 7))
    sc.score(_capi.EIG)
    ids, score, total, _, _ = sc.rank(1, 0, max_out=N)
    assert 64 * 200 < total == ids.shape[0] < N
    order = np.concatenate([ids, np.setdiff1d(np.arange(N), ids)])      # the ranking, then the candidates that are not violated
    Sp, kp, coef, el = pool_rows(sc, S, ks, order)
    assert el[:total].all() and not el[total:].any()
    for quota, mp in ((N, 0.1), (600, 0.5), (1000, 0.9)):
        keep_t, info_t = diversity.greedy_filter(Sp, kp, coef, el, quota, mp, return_info=True)
        closest = info_t.pop("closest")
        print("pool %d quota %d max_parallel %.1f: %s, closest pair %.3e from the threshold" % (N, quota, mp, info_t, closest))
        assert closest > MARGIN
        keep_d, info_d = sc.filter_parallel(order, quota, mp)
        assert np.array_equal(keep_d, keep_t) and info_d == info_t, (quota, mp)
        if quota <= N // 4:
            r = sc.round_csr_diverse(None, 1, quota, mp, pool_size=N)
            assert np.array_equal(r["idx"], order[keep_t]) and r["info"]["pool"] == total
            assert r["info"]["examined"] == min(info_t["examined"], total)


def test_emitted_rows_are_the_rows_of_cut_rows(scorers):
    """the CSR block of a filtered round: values and columns of every accepted entry are those sdpcut_cut_rows gives, bit for bit"""
    sc, _ = scorers
    n, S, ks = bind(sc, "mixed")
    vv = random_point(n, 7)
    r = sc.round_csr_diverse(vv, 1, 60, 0.5, copy=True)
    assert 0 < r["idx"].shape[0] <= 60 and r["info"]["rejected_parallel"] > 0
    lam, coef, rhs, cols, kk = sc.cut_rows(r["idx"] - sc.base)
    assert np.array_equal(lam, r["lam"]) and np.array_equal(rhs, r["rhs"]) and np.array_equal(kk, r["ks"])
    for c in range(r["idx"].shape[0]):
        lo, hi = r["indptr"][c], r["indptr"][c + 1]
        w = int(kk[c]) * (int(kk[c]) + 3) // 2
        assert hi - lo == w and np.array_equal(r["values"][lo:hi], coef[c, :w]) and np.array_equal(r["indices"][lo:hi], cols[c, :w])


# ------------------------------------------------------------------------------------------ 3. the structured vertex
@pytest.mark.parametrize("strat", [1, 4])
def test_structured_vertex_invariants(scorers, strat):
    from sdpcutsel_via_nn_amd import diversity
    sc, _ = scorers
    inst, S, ks = boxqp_cover("spar020-100-1.in", 3)
    bind(sc, "spar020")
    sc.set_point(mccormick_vertex(inst))
    sc.score(FLAGS[strat])
    for quota in (37, 100):
        ids, score, total, _, _ = sc.rank(strat, quota, max_out=S.shape[0])
        loc = ids - sc.base
        Sp, kp, coef, el = pool_rows(sc, S, ks, loc)
        cos = diversity.pair_cosines(Sp, kp, coef)
        for mp in (0.1, 0.5, 0.9):
            for pool in (quota, 257, S.shape[0]):
                P = min(pool, ids.shape[0])
                keep, info = sc.filter_parallel(loc[:P], quota, mp)
                assert diversity.check_walk(Sp[:P], kp[:P], coef[:P], el[:P], quota, mp, keep, margin=MARGIN, examined=info["examined"], cos=cos)
                assert info["examined"] == keep.sum() + info["skipped_nonviolated"] + info["rejected_parallel"]
                r = sc.round_csr_diverse(None, strat, quota, mp, pool_size=pool)
                # the round walks the same pool in the same order: an answer that passes the same check
                pos = {int(g): i for i, g in enumerate(ids[:P])}
                keep_r = np.zeros(P, dtype=bool)
                keep_r[[pos[int(g)] for g in r["idx"]]] = True
                assert np.array_equal(np.flatnonzero(keep_r), np.sort(np.flatnonzero(keep_r))) and keep_r.sum() == r["idx"].shape[0]
                assert np.array_equal(ids[:P][keep_r], r["idx"])      # rank order
                assert diversity.check_walk(Sp[:P], kp[:P], coef[:P], el[:P], quota, mp, keep_r, margin=MARGIN,
                                            examined=r["info"]["examined"], cos=cos)


# ------------------------------------------------------------------------------------------ 4. edges of the walk
def test_quota_inside_a_block_short_pool_and_no_eligible_entry(scorers):
    sc, fresh = scorers
    n, S, ks = bind(sc, "spar020")
    vv = random_point(n, 7)
    # the quota fills in the middle of a block of 64: the walk ends there
    r = sc.round_csr_diverse(vv, 1, 37, 0.5, pool_size=1000)
    assert r["idx"].shape[0] == 37 and r["info"]["examined"] % 64 != 0 and r["info"]["examined"] < r["info"]["pool"]
    assert r["info"]["examined"] == 37 + r["info"]["skipped_nonviolated"] + r["info"]["rejected_parallel"]
    # a pool shorter than the quota: everything is examined
    n2, S2, ks2 = bind(sc, "mixed")
    vv2 = random_point(n2, 7)
    r = sc.round_csr_diverse(vv2, 1, 500, 0.9, pool_size=600)
    assert r["info"]["pool"] == r["n_total"] <= S2.shape[0] < 500 and r["info"]["examined"] == r["info"]["pool"]
    assert 0 < r["idx"].shape[0] < 500
    keep, info = sc.filter_parallel(np.arange(50), 64, 0.9)
    assert info["pool"] == 50 and (info["examined"] == 50 or keep.sum() == 64)
    # no eligible entry: a PSD point, X = min(x_i, x_j)
    x = np.random.default_rng(3).uniform(0.05, 0.95, n2)
    iu = np.triu_indices(n2)
    psd = np.concatenate([np.minimum(x[iu[0]], x[iu[1]]), x])
    for strat in (1, 2, 4):
        r = sc.round_csr_diverse(psd, strat, 40, 0.5)
        assert r["idx"].shape[0] == 0 and r["rhs"].shape[0] == 0 and r["indices"].shape[0] == 0 and r["indptr"].tolist() == [0]
        want_pool = 0 if strat == 1 else min(160, S2.shape[0])
        assert r["info"] == dict(pool=want_pool, examined=want_pool, skipped_nonviolated=want_pool, rejected_parallel=0)
    keep, info = sc.filter_parallel(np.arange(S2.shape[0]), 10, 0.5)
    assert not keep.any() and info["skipped_nonviolated"] == S2.shape[0]
    # nothing was left behind: a plain round on this handle is the plain round of a fresh handle
    bind(fresh, "mixed")
    for strat in (4, 1, 2):
        got = sc.round_csr(strat, 60, point=vv2, copy=True)
        want = fresh.round_csr(strat, 60, point=vv2, copy=True)
        for f in ARRAYS:
            assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (strat, f)
        assert (got["n_total"], got["new_strat"], got["counters"]) == (want["n_total"], want["new_strat"], want["counters"])


def test_refusals(scorers):
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import _capi
    sc, _ = scorers
    n, S, ks = bind(sc, "spar020")
    vv = random_point(n, 7)
    lib, h = sc._lib, sc._h
    out, info = _capi.RoundCsr(), _capi.DiverseInfo()
    import ctypes
    p = vv.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def call(strat=1, sel=10, pool=40, mp=0.5):
        return lib.sdpcut_round_csr_diverse(h, p, strat, sel, pool, mp, ctypes.byref(out), ctypes.byref(info))
    assert call() == 0
    for kw in (dict(strat=0), dict(strat=3), dict(strat=5), dict(strat=104), dict(mp=-0.01), dict(mp=1.01), dict(mp=float("nan")),
               dict(sel=0), dict(pool=9), dict(sel=10, pool=_capi.DIVERSE_MAX_POOL + 1)):
        assert call(**kw) == -1, kw      # SDPCUT_EINVAL
    ids = np.zeros(_capi.DIVERSE_MAX_POOL + 1, dtype=np.int64)
    keep = np.zeros(ids.shape[0], dtype=np.uint8)
    i64p, u8p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint8)
    assert lib.sdpcut_filter_parallel(h, ids.shape[0], ids.ctypes.data_as(i64p), 5, 0.5, keep.ctypes.data_as(u8p), None) == -1
    bad = np.array([0, S.shape[0]], dtype=np.int64)
    assert lib.sdpcut_filter_parallel(h, 2, bad.ctypes.data_as(i64p), 5, 0.5, keep.ctypes.data_as(u8p), None) == -1
    # state: a round pending; no point; no candidates
    sc.round_csr_begin(1, 10, point=vv)
    assert call() == -4 and lib.sdpcut_filter_parallel(h, 2, ids.ctypes.data_as(i64p), 5, 0.5, keep.ctypes.data_as(u8p), None) == -4
    sc.round_csr_end()
    empty = pkg.Scorer(0)
    try:
        assert lib.sdpcut_round_csr_diverse(empty._h, None, 1, 10, 40, 0.5, ctypes.byref(out), ctypes.byref(info)) == -4
        empty.set_instance(n, np.zeros(n * (n + 1) // 2))
        assert lib.sdpcut_round_csr_diverse(empty._h, p, 1, 10, 40, 0.5, ctypes.byref(out), ctypes.byref(info)) == -4
        empty.set_candidates(S, ks)
        assert lib.sdpcut_round_csr_diverse(empty._h, None, 1, 10, 40, 0.5, ctypes.byref(out), ctypes.byref(info)) == -4
        assert lib.sdpcut_filter_parallel(empty._h, 2, ids.ctypes.data_as(i64p), 5, 0.5, keep.ctypes.data_as(u8p), None) == -4
    finally:
        empty.close()


# ------------------------------------------------------------------------------------------ 5. the loop
def test_cutting_plane_loop_with_the_filter():
    from sdpcutsel_via_nn_amd.cut_solver import CutSolver
    path = os.path.join(INST, "spar020-100-1.in")
    seen = []
    solver = CutSolver()

    def on_round(r, log):
        lp = solver._my_prob
        seen.append((np.array(lp.get_values(), dtype=np.float64), lp.linear_constraints.get_num()))
    out = solver.cut_select_algo(path, 3, 0.1, strat=1, nb_rounds_cuts=2, max_parallel=0.5, on_round=on_round)
    bounds, cuts, n_cand = out[0], out[4], out[6]
    quota = CutSolver.selection_size(0.1, n_cand)
    assert len(bounds) == 3 and len(seen) == 3 and len(solver.diverse_log) == 2
    assert cuts[0] == 0 and all(0 < c <= quota for c in cuts[1:]), cuts
    assert bounds[2] <= bounds[1] <= bounds[0]      # (upper bounds of the maximisation: every round tightens)
    store = solver._my_prob.linear_constraints
    n, L = 20, 210
    rng = np.random.default_rng(0)
    xs = rng.uniform(0.0, 1.0, (100, n))
    iu = np.triu_indices(n)
    rank_one = np.concatenate([xs[:, iu[0]] * xs[:, iu[1]], xs], axis=1)      # [X = x x^T packed | x]
    for r in (1, 2):
        point, first = seen[r - 1]
        last = seen[r][1]
        assert last - first == cuts[r] == solver.diverse_log[r - 1]["accepted"]
        data, cols, lens = store.csr_parts(first)
        rhs = store.rhs_from(first)
        ptr = np.concatenate([[0], np.cumsum(lens)])
        for c in range(cuts[r]):
            a, j = data[ptr[c]:ptr[c + 1]], cols[ptr[c]:ptr[c + 1]]
            assert a @ point[j] < rhs[c], (r, c)                          # violated at the point it was cut from
            assert (rank_one[:, j] @ a >= rhs[c] - 1e-9).all(), (r, c)    # valid for every (x, x x^T)
    # off by default, and None is the path as it was: the same bounds and cut counts as a run without the argument
    plain = CutSolver().cut_select_algo(path, 3, 0.1, strat=1, nb_rounds_cuts=2)
    none = CutSolver().cut_select_algo(path, 3, 0.1, strat=1, nb_rounds_cuts=2, max_parallel=None)
    assert len(none) == len(plain) == 7
    for i in (0, 4, 5, 6):      # (entries 1-3 are wall-clock times)
        assert none[i] == plain[i], i
    with pytest.raises(AssertionError):
        CutSolver().cut_select_algo(path, 3, 0.1, strat=0, nb_rounds_cuts=1, max_parallel=0.5)
