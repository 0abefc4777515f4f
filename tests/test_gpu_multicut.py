"""All violated eigen-cuts of a selected set on the device (sdpcut_round_csr_multi, sdpcut_cut_rows_all; csrc/multirows.hip) against
the numpy twin (sdpcutsel_via_nn_amd/multicut.py: numpy.linalg.eigh per head entry, then the walk).

Inputs: spar020-100-1 (n = 20) with lists bound through set_candidates, at random_mccormick_point(20, seed 7 / 8):
  tri    all 1140 3-subsets;   quad   the first 2048 4-subsets;
  mixed  2-, 3-, 4- and 5-subsets interleaved so that one wave holds all sizes: 300 each of the sizes 3, 4, 5 and ALL 190 pairs (20
         variables have no 300 distinct pairs, and a repeated set would tie its ranking key with its twin's).
Bounds: row_lam 2e-13 (the project's lambda_min bound), values / rhs 1e-9 (its rows bound); everything else exact.  Every
comparison with the twin FIRST asserts on the twin what makes it meaningful: eigenvalues of one matrix >= 1e-5 apart (the
eigenvector error is then <= 1e-10), no eigenvalue within 1e-9 of the threshold -1e-15 (so both sides count the same violated
eigenvalues), neighbouring ranking scores of the head >= 1e-12 apart, and at least 30 % of the walked entries offering two rows or
more.  (Measured with the twin: the heads by lambda_min hold 40-88 % such entries -- except tri at seed 7, whose head of 500 holds
23 %: that list is compared at seed 8, and at seed 7 with heads up to 129.)  At the structured vertex eigenvalues tie, so the
answer is checked against the invariants of multicut.check_rows instead."""
import ctypes
import itertools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INST = os.path.join(ROOT, "tests", "golden", "instances", "spar020-100-1.in")
N = 20
HEAD = ("idx", "score", "ks", "set_inds")
PLAIN = ("idx", "score", "lam", "ks", "set_inds", "row_entry", "indptr", "indices", "values", "rhs")
MULTI = PLAIN + ("n_neg", "row_lam", "row_rank")
LAM_TOL, ROW_TOL = 2e-13, 1e-9
_cache = {}


def instance():
    from sdpcutsel_via_nn_amd import harness
    if "inst" not in _cache:
        _cache["inst"] = harness.parse_boxqp(INST)
    return _cache["inst"]


def the_list(name):
    if name not in _cache:
        if name == "tri":
            sets = list(itertools.combinations(range(N), 3))
        elif name == "quad":
            sets = list(itertools.islice(itertools.combinations(range(N), 4), 2048))
        else:
            parts = [list(itertools.islice(itertools.combinations(range(N), k), 300)) for k in (2, 3, 4, 5)]
            sets = [p[i] for i in range(300) for p in parts if i < len(p)]
        S = np.full((len(sets), 5), -1, dtype=np.int32)
        for i, s in enumerate(sets):
            S[i, :len(s)] = s
        _cache[name] = (S, np.array([len(s) for s in sets], dtype=np.int32))
    return _cache[name]


def point(seed):
    from sdpcutsel_via_nn_amd import harness
    if ("pt", seed) not in _cache:
        _cache[("pt", seed)] = harness.random_mccormick_point(N, np.random.default_rng(seed))
    return _cache[("pt", seed)]


def vertex():
    """the optimum of the McCormick relaxation: x = 0.5, X_ii = 0.5, X_ij in {0, 0.5} by the sign of q_ij"""
    Q = np.asarray(instance()["Q_arr"], dtype=np.float64)
    X = np.where(Q < 0, 0.5, 0.0)
    iu = np.triu_indices(N)
    X[iu[0] == iu[1]] = 0.5
    return np.concatenate([X, np.full(N, 0.5)])


@pytest.fixture(scope="module")
def scorers():
    import sdpcutsel_via_nn_amd as pkg
    scs = []
    for _ in range(2):
        sc = pkg.Scorer(0)
        sc.set_builtin_networks(5)
        scs.append(sc)
    yield tuple(scs)
    for sc in scs:
        sc.close()


def bind(sc, name):
    sc.drop_pending()
    S, ks = the_list(name)
    sc.set_instance(N, np.asarray(instance()["Q_arr"], dtype=np.float64))
    sc.set_candidates(S, ks)
    return S, ks


def twin(name, seed, vv, idx, m):
    """multicut.expected for the head `idx` of list `name` (computed once per head and m)"""
    from sdpcutsel_via_nn_amd import multicut
    key = ("twin", name, seed, m, idx.tobytes())
    if key not in _cache:
        S, ks = the_list(name)
        _cache[key] = multicut.expected(S[idx], ks[idx], vv, N, m)
    return _cache[key]


def assert_preconditions(e, plain, share=True):
    gaps = min(float(np.diff(w).min()) for w in e["eigvals"])
    thr = min(float(np.abs(w + 1e-15).min()) for w in e["eigvals"])
    assert gaps >= 1e-5, "eigenvalues of one matrix %.2e apart: the twin's vectors are not comparable" % gaps
    assert thr >= 1e-9, "an eigenvalue %.2e from the threshold" % thr
    if plain["score"].shape[0] > 1:
        assert np.abs(np.diff(plain["score"])).min() >= 1e-12, "neighbouring ranking scores tie"
    if share:
        used = np.flatnonzero(e["n_offered"] > 0)
        walked = e["n_offered"][:int(used[-1]) + 1] if used.size else e["n_offered"]
        assert walked.shape[0] and (walked >= 2).mean() >= 0.30, "%.0f %% of the walked entries offer two rows" % (100 * (walked >= 2).mean())


def assert_round_equals_twin(res, plain, e, quota, m, cap):
    from sdpcutsel_via_nn_amd import multicut
    t = multicut.apply_walk(e, quota)
    for f in HEAD:
        assert res[f].dtype == plain[f].dtype and np.array_equal(res[f], plain[f]), f
    assert (res["n_total"], res["new_strat"], res["counters"]) == (plain["n_total"], plain["new_strat"], plain["counters"])
    assert np.array_equal(res["n_neg"], e["n_neg"])
    for f in ("row_entry", "row_rank", "indptr", "indices"):
        assert res[f].dtype == np.int32 and np.array_equal(res[f], t[f]), (f, quota, m)
    assert (res["n_used"], res["quota_hit"]) == (t["n_used"], t["quota_hit"]), (quota, m)
    assert res["row_cap"] == min(quota, m * cap)
    assert np.abs(res["lam"] - e["lam_min"]).max() <= LAM_TOL
    if t["n_rows"]:
        assert np.abs(res["row_lam"] - t["row_lam"]).max() <= LAM_TOL
        assert np.abs(res["values"] - t["values"]).max() <= ROW_TOL and np.abs(res["rhs"] - t["rhs"]).max() <= ROW_TOL
    return t


def quota_inside_an_entry(e, cap):
    """a quota that ends inside an entry behind the first workgroup where the head has one (the look-back carries the count)"""
    off = e["n_offered"]
    cand = np.flatnonzero(off >= 2)
    assert cand.size
    pick = cand[cand <= max(int(0.6 * cap), int(cand[0]))][-1]
    return int(off[:pick].sum()) + 1


# ------------------------------------------------------------------------------------------ 1. m = 1 is the plain round
@pytest.mark.parametrize("strat", [1, 2, 4])
@pytest.mark.parametrize("name,seed", [("tri", 7), ("mixed", 8)])
def test_one_cut_per_set_is_the_plain_round(scorers, name, seed, strat):
    sc, fresh = scorers
    bind(sc, name)
    bind(fresh, name)
    vv = point(seed)
    for sel in (64, 129, 500):
        a = fresh.round_csr(strat, sel, point=vv, copy=True)
        r = sc.round_csr_multi(vv, strat, sel, 1, copy=True)
        assert a["rhs"].shape[0] > 0
        for f in PLAIN:
            assert r[f].dtype == a[f].dtype and np.array_equal(r[f], a[f]), (sel, f)
        assert (r["n_total"], r["new_strat"], r["counters"]) == (a["n_total"], a["new_strat"], a["counters"])
        assert np.array_equal(r["row_lam"], a["lam"][a["row_entry"]]) and not r["row_rank"].any()
        assert np.array_equal(r["n_neg"], (a["lam"] < -1e-15).astype(np.int32))
        assert r["n_used"] == int(a["row_entry"][-1]) + 1 and not r["quota_hit"]
        # the quota on the forwarded round: a prefix
        q = a["rhs"].shape[0] - 3
        c = sc.round_csr_multi(vv, strat, sel, 1, row_quota=q, copy=True)
        assert c["quota_hit"] and c["rhs"].shape[0] == q and np.array_equal(c["values"], a["values"][:a["indptr"][q]])
        assert np.array_equal(c["indptr"], a["indptr"][:q + 1]) and c["n_used"] == int(a["row_entry"][q - 1]) + 1


# ------------------------------------------------------------------------------------------ 2. m = 2, 3, 5 against the twin
TWIN_CASES = [("tri", 8, 1, (64, 65, 129, 500)), ("tri", 7, 1, (64, 65, 129)), ("quad", 7, 1, (64, 65, 129, 500)),
              ("quad", 8, 4, (64, 65, 129, 500)), ("mixed", 7, 1, (64, 65, 129, 500)), ("mixed", 8, 4, (64, 65, 129, 500))]


@pytest.mark.parametrize("name,seed,strat,heads", TWIN_CASES)
def test_rows_equal_the_twin(scorers, name, seed, strat, heads):
    sc, _ = scorers
    bind(sc, name)
    vv = point(seed)
    walked_inside = 0
    for cap in heads:
        plain = sc.round_csr(strat, cap, point=vv, copy=True)
        idx = plain["idx"]
        assert idx.shape[0] == cap, "the head is shorter than asked for: choose another case"
        for m in (2, 3, 5):
            e = twin(name, seed, vv, idx, m)
            assert_preconditions(e, plain)
            inside = quota_inside_an_entry(e, cap)
            for quota in (cap, m * cap, 1, inside):
                res = sc.round_csr_multi(vv, strat, cap, m, row_quota=quota, copy=True)
                t = assert_round_equals_twin(res, plain, e, quota, m, cap)
                if quota == inside:
                    last = int(t["row_entry"][-1])
                    assert t["kept"][last] < e["n_offered"][last] and t["quota_hit"], "the quota does not end inside an entry"
                    walked_inside += last >= 32
            # the named forms of the quota
            assert sc.round_csr_multi(vv, strat, cap, m)["rhs"].shape[0] == min(cap, int(e["n_offered"].sum()))
            full = sc.round_csr_multi(vv, strat, cap, m, row_quota="sets")
            assert full["rhs"].shape[0] == int(e["n_offered"].sum()) and not full["quota_hit"]
    assert walked_inside > 0, "no quota ended behind the first workgroup"


# ------------------------------------------------------------------------------------------ 3. entries without a cut inside the head
@pytest.mark.parametrize("name,seed", [("tri", 7), ("mixed", 8)])
def test_optimality_head_with_non_violated_entries(scorers, name, seed):
    """strategy 2 ranks by the estimated objective improvement: its head holds entries with no violated eigenvalue, which emit
    nothing; the rows behind them land where the twin says.  (No 30 % condition here: the precondition is the gaps in the head.)"""
    sc, _ = scorers
    bind(sc, name)
    vv = point(seed)
    for cap in (129, 500):
        plain = sc.round_csr(2, cap, point=vv, copy=True)
        for m in (2, 5):
            e = twin(name, seed, vv, plain["idx"], m)
            assert_preconditions(e, plain, share=False)
            none = np.flatnonzero(e["n_offered"] == 0)
            some = np.flatnonzero(e["n_offered"] > 0)
            assert none.size >= 5 and some.size and none[0] < some[-1], "no entry without a cut in front of one with cuts"
            for quota in (cap, m * cap, quota_inside_an_entry(e, cap)):
                res = sc.round_csr_multi(vv, 2, cap, m, row_quota=quota, copy=True)
                assert_round_equals_twin(res, plain, e, quota, m, cap)
                assert not np.isin(res["row_entry"], none).any()


# ------------------------------------------------------------------------------------------ 4. the structured vertex
def test_structured_vertex_by_invariants(scorers):
    from sdpcutsel_via_nn_amd import multicut
    sc, _ = scorers
    S, ks = bind(sc, "tri")
    vv = vertex()
    for cap, m, quota in ((500, 5, 2500), (129, 2, 129), (500, 3, 700)):
        plain = sc.round_csr(1, cap, point=vv, copy=True)
        res = sc.round_csr_multi(vv, 1, cap, m, row_quota=quota, copy=True)
        idx = res["idx"]
        assert idx.shape[0] > 0 and np.array_equal(idx, plain["idx"]) and np.array_equal(res["score"], plain["score"])
        rows = res["rhs"].shape[0]
        assert rows > 0
        coef = np.zeros((rows, 20))
        for r in range(rows):
            lo, hi = res["indptr"][r], res["indptr"][r + 1]
            coef[r, :hi - lo] = res["values"][lo:hi]
            _, cols = multicut.lifted(S[idx[res["row_entry"][r]], :3], vv, N)
            assert np.array_equal(res["indices"][lo:hi], cols)
        assert multicut.check_rows(S[idx], ks[idx], vv, N, m, res["row_entry"], res["row_rank"], res["row_lam"], coef, res["rhs"],
                                   row_quota=quota)
        assert res["n_used"] == (int(res["row_entry"][-1]) + 1) and res["quota_hit"] == (rows == quota and res["n_neg"].clip(max=m).sum() > quota)


# ------------------------------------------------------------------------------------------ 5. an explicit id list
@pytest.mark.parametrize("seed", [7, 8])
def test_cut_rows_all(scorers, seed):
    from sdpcutsel_via_nn_amd import multicut
    sc, _ = scorers
    S, ks = bind(sc, "mixed")
    vv = point(seed)
    sc.set_point(vv)
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, S.shape[0], 1000)
    ids[500] = ids[3]
    assert np.unique(ids).shape[0] < 1000
    # m = 1: the rows of cut_rows where lam_min is violated, bit for bit
    lam, coef, rhs, cols, kk = sc.cut_rows(ids)
    rp, rl, co, rh, cl, k1 = sc.cut_rows_all(ids, 1)
    sel = lam < -1e-15
    assert 0 < sel.sum() < 1000
    assert np.array_equal(rp, np.concatenate([[0], np.cumsum(sel)])) and rp.dtype == np.int64
    assert np.array_equal(rl, lam[sel]) and np.array_equal(co, coef[sel]) and np.array_equal(rh, rhs[sel])
    assert np.array_equal(cl, cols) and np.array_equal(k1, kk) and np.array_equal(kk, ks[ids])
    # m = 5 against the twin
    e = multicut.expected(S[ids], ks[ids], vv, N, 5)
    assert min(float(np.diff(w).min()) for w in e["eigvals"]) >= 1e-5 and min(float(np.abs(w + 1e-15).min()) for w in e["eigvals"]) >= 1e-9
    assert (e["n_offered"] >= 2).mean() >= 0.2
    rp, rl, co, rh, cl, k5 = sc.cut_rows_all(ids, 5)
    assert np.array_equal(rp, np.concatenate([[0], np.cumsum(e["n_offered"])]))
    assert np.array_equal(k5, ks[ids]) and np.array_equal(cl, cols)
    assert np.abs(rl - e["row_lam"]).max() <= LAM_TOL
    assert np.abs(co - e["coef"]).max() <= ROW_TOL and np.abs(rh - e["rhs"]).max() <= ROW_TOL
    # the same entries through the round: identical rows
    for cap, m in ((129, 5), (500, 3)):
        r = sc.round_csr_multi(vv, 1, cap, m, row_quota="sets", copy=True)
        rp, rl, co, rh, cl, kk = sc.cut_rows_all(r["idx"], m)
        assert np.array_equal(np.diff(rp), np.minimum(r["n_neg"], m)) and rp[-1] == r["rhs"].shape[0] > cap // 2
        assert np.array_equal(rl, r["row_lam"]) and np.array_equal(rh, r["rhs"])
        for row in range(int(rp[-1])):
            lo, hi = r["indptr"][row], r["indptr"][row + 1]
            ent = r["row_entry"][row]
            assert np.array_equal(co[row, :hi - lo], r["values"][lo:hi]) and not co[row, hi - lo:].any()
            assert np.array_equal(cl[ent, :hi - lo], r["indices"][lo:hi])


# ------------------------------------------------------------------------------------------ 6. repeatability
def test_two_handles_give_the_same_bits(scorers):
    a, b = scorers
    for name, seed, strat, cap, m, quota in (("mixed", 7, 4, 129, 3, 200), ("quad", 8, 1, 500, 5, "sets"), ("tri", 7, 2, 65, 2, None)):
        bind(a, name)
        bind(b, name)
        vv = point(seed)
        ra = a.round_csr_multi(vv, strat, cap, m, row_quota=quota, copy=True)
        rb = b.round_csr_multi(vv, strat, cap, m, row_quota=quota, copy=True)
        again = a.round_csr_multi(None, strat, cap, m, row_quota=quota, copy=True)      # the current point, scores in place
        assert ra["rhs"].shape[0] > 0
        for other in (rb, again):
            for f in MULTI:
                assert np.array_equal(ra[f], other[f], equal_nan=True), (name, f)
            for f in ("n_total", "new_strat", "counters", "n_used", "quota_hit", "row_cap"):
                assert ra[f] == other[f], (name, f)


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_handle_usable(scorers):
    from sdpcutsel_via_nn_amd import _capi
    sc, _ = scorers
    S, ks = bind(sc, "tri")
    vv = point(7)
    sc.set_point(vv)
    lib, h = sc._lib, sc._h
    out = _capi.RoundMulti()
    EINVAL, ESTATE = -1, -4

    def call(strat, sel, m, quota):
        return lib.sdpcut_round_csr_multi(h, None, strat, sel, m, quota, ctypes.byref(out))
    assert call(1, 64, 0, 64) == EINVAL and call(1, 64, 6, 64) == EINVAL
    assert call(1, 64, 2, 0) == EINVAL and call(1, 64, 1, 0) == EINVAL
    assert call(0, 64, 2, 64) == EINVAL and call(5, 64, 2, 64) == EINVAL and call(-1, 64, 2, 64) == EINVAL
    assert call(3, 64, 2, 64) == EINVAL      # strategy 3 without SDPCUT_OPT_EXACT_SDP, as the plain round refuses it
    assert call(1, -1, 2, 64) == EINVAL
    assert out.csr.cap == 0 and not out.csr.idx and not out.n_neg
    ids = np.arange(10, dtype=np.int64)
    i64, dbl, i32 = (ctypes.POINTER(t) for t in (ctypes.c_int64, ctypes.c_double, ctypes.c_int32))
    rp, lam, co, rh = np.zeros(11, np.int64), np.zeros(60), np.zeros((60, 20)), np.zeros(60)
    cl, kk = np.zeros((10, 20), np.int64), np.zeros(10, np.int32)

    def rows_all(m, idv=ids):
        return lib.sdpcut_cut_rows_all(h, 10, idv.ctypes.data_as(i64), m, rp.ctypes.data_as(i64), lam.ctypes.data_as(dbl), co.ctypes.data_as(dbl),
                                       rh.ctypes.data_as(dbl), cl.ctypes.data_as(i64), kk.ctypes.data_as(i32))
    assert rows_all(0) == EINVAL and rows_all(6) == EINVAL
    assert rows_all(2, np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, S.shape[0]], dtype=np.int64)) == EINVAL
    assert rows_all(2, np.array([0, 1, 2, 3, -1, 5, 6, 7, 8, 9], dtype=np.int64)) == EINVAL
    # the Python layer says the same before it calls
    for bad in (dict(cuts_per_set=0), dict(cuts_per_set=6), dict(cuts_per_set=2, row_quota=0)):
        with pytest.raises(ValueError):
            sc.round_csr_multi(vv, 1, 64, **bad)
    for strat in (0, 5):
        with pytest.raises(ValueError):
            sc.round_csr_multi(vv, strat, 64, 2)
    # a round begun and not ended
    sc.round_csr_begin(1, 64, point=vv)
    assert call(1, 64, 2, 64) == ESTATE and call(1, 64, 1, 64) == ESTATE and rows_all(2) == ESTATE
    pend = sc.round_csr_end(copy=True)
    # the plain round, and the multi round, still work on this handle
    a = sc.round_csr(1, 64, point=vv, copy=True)
    for f in PLAIN:
        assert np.array_equal(a[f], pend[f]), f
    r = sc.round_csr_multi(vv, 1, 64, 2)
    assert np.array_equal(r["idx"], a["idx"]) and r["rhs"].shape[0] == 64 and r["quota_hit"]
    assert rows_all(2) == 0 and rp[10] > 0


# ------------------------------------------------------------------------------------------ 8. the solver's rounds
def test_cut_solver_rounds_with_all_violated_cuts():
    import sdpcutsel_via_nn_amd as pkg
    one = pkg.CutSolver()
    b1, _, _, _, sdp1, _, n_cand = one.cut_select_algo(INST, 4, 0.1, strat=1, nb_rounds_cuts=2)
    assert getattr(one, "multi_log", None) is None
    again = pkg.CutSolver()
    b1b, _, _, _, sdp1b, _, _ = again.cut_select_algo(INST, 4, 0.1, strat=1, nb_rounds_cuts=2, cuts_per_set=1)
    assert sdp1b == sdp1 and b1b == b1 and getattr(again, "multi_log", None) is None      # the default is today's path
    quota = pkg.CutSolver.selection_size(0.1, n_cand)
    assert sdp1[1] == quota
    cs = pkg.CutSolver()
    b5, _, _, _, sdp5, _, n5 = cs.cut_select_algo(INST, 4, 0.1, strat=1, nb_rounds_cuts=2, cuts_per_set=5)
    assert n5 == n_cand and len(cs.multi_log) == 2 and cs.cuts_per_set == 1
    mccormick = b5[0]
    assert mccormick == b1[0] and b1[-1] != b1[0]
    better = np.sign(b1[-1] - b1[0])      # the direction in which the plain run's cuts move the reported bound
    for rnd, rec in enumerate(cs.multi_log):
        assert rec["rows"] == sdp5[rnd + 1] <= quota and rec["quota"] == quota
        assert rec["entries"] == quota and rec["entries_used"] <= rec["last_entry"] <= rec["entries"]
        assert sum(rec["n_neg_hist"]) == rec["entries"] and rec["round"] == rnd + 1 and rec["strat"] == 1
        offered = sum(min(j, 5) * c for j, c in enumerate(rec["n_neg_hist"]))
        assert rec["quota_hit"] == (offered > quota)
        # every round's bound is no worse than McCormick's
        assert (b5[rnd + 1] - mccormick) * better >= -1e-9 * abs(mccormick)
    assert cs.multi_log[0]["entries_used"] < cs.multi_log[0]["rows"], "round 1 uses fewer sets than rows"
    # the set budget: every selected set keeps what it offers
    cs2 = pkg.CutSolver()
    _, _, _, _, sdps, _, _ = cs2.cut_select_algo(INST, 4, 0.1, strat=1, nb_rounds_cuts=1, cuts_per_set=5, row_quota="sets")
    rec = cs2.multi_log[0]
    assert sdps[1] == rec["rows"] == sum(min(j, 5) * c for j, c in enumerate(rec["n_neg_hist"])) > quota and not rec["quota_hit"]
    # strategy 5 goes through cut_rows_all behind the attribute
    cs3 = pkg.CutSolver()
    _, _, _, _, sdpr, _, _ = cs3.cut_select_algo(INST, 4, 0.1, strat=5, nb_rounds_cuts=1, cuts_per_set=5)
    rec = cs3.multi_log[0]
    assert sdpr[1] == rec["rows"] <= quota and rec["entries"] == quota and sum(rec["offered_hist"]) == quota
