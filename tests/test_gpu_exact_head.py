"""SDPCUT_OPT_EXACT_HEAD: heads of the NN-ranked strategies (2 = optimality, 4 = combined) ordered and reported by obj_improve in
the reference's operation order.  The checker is the CPU oracle: obj_exact = oracle.opt_score_batch for EVERY candidate, eig_dev
the device's lambda_min, and the head must be oracle.rank_arrays(strat, obj_exact, eig_dev, sel) position by position, the scores
bit for bit."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

EINVAL_TEXT = "8192"


def _instance(name):
    from sdpcutsel_via_nn_amd import harness
    return harness.parse_boxqp(os.path.join(GOLDEN, "instances", name + ".in"))


def _point(n, seed):
    """a generic point [X packed | x]: x in (0, 1), X = x x^T + noise (some candidates violated, some not)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.05, 0.95, n)
    X = np.outer(x, x) + 0.08 * rng.standard_normal((n, n))
    X = 0.5 * (X + X.T)
    iu = np.triu_indices(n)
    return np.concatenate([X[iu], x])


def _obj_exact(oracle, S, ks, n, vv, Q):
    out = np.empty(S.shape[0])
    for k in np.unique(ks):
        m = ks == k
        out[m] = oracle.opt_score_batch(int(k), S[m][:, :k], n, vv, Q)
    return out


def _scorer(n, Q, S, ks, exact=True):
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import _capi
    sc = pkg.Scorer(0)
    sc.set_builtin_networks(5)
    sc.set_instance(n, Q)
    sc.set_candidates(S, ks)
    sc.set_option(_capi.OPT_EXACT_HEAD, 1 if exact else 0)
    return sc


class _List(object):
    """one candidate list at one point with the oracle's exact scores, computed once and shared by the tests"""

    def __init__(self, oracle, n, Q, S, ks, vv):
        self.n, self.Q, self.S, self.ks, self.vv = n, np.asarray(Q, dtype=np.float64), S, ks, vv
        self.obj = _obj_exact(oracle, S, ks, n, vv, self.Q)


@pytest.fixture(scope="module")
def small(oracle, golden_boxqp):
    """spar020-100-1 dim 3: 1051 candidates (below SDPCUT_PF_MIN_N, one-workgroup routes), head 105"""
    g, t = golden_boxqp, "spar020_100_1_d3_"
    S = np.ascontiguousarray(g[t + "set_inds"], dtype=np.int32)
    return _List(oracle, int(g[t + "nb_vars"]), g[t + "Q_arr"], S, np.ascontiguousarray(g[t + "k"], dtype=np.int32), g[t + "rnd_vars"])


@pytest.fixture(scope="module")
def big(oracle):
    """40 000 triples drawn with replacement on spar100-050-1 (n = 100; above SDPCUT_PF_MIN_N, the radix routes), head 5000"""
    inst = _instance("spar100-050-1")
    n = inst["nb_vars"]
    rng = np.random.default_rng(11)
    S = np.sort(np.array([rng.choice(n, 3, replace=False) for _ in range(4000)]), axis=1)
    S = np.ascontiguousarray(S[rng.integers(0, 4000, 40000)], dtype=np.int32)      # with replacement: equal scores, ties by index
    S5 = np.full((40000, 5), -1, dtype=np.int32)
    S5[:, :3] = S
    return _List(oracle, n, inst["Q_arr"], S5, np.full(40000, 3, dtype=np.int32), _point(n, 3))


def _check_head(oracle, sc, L, strat, sel, res, eig_dev):
    order, score, new_strat, cnt = oracle.rank_arrays(strat, L.obj, eig_dev, sel)
    w = min(sel, L.S.shape[0])
    assert res["idx"].shape[0] == w
    assert np.array_equal(res["idx"], order[:w]), np.flatnonzero(res["idx"] != order[:w])[:5]
    assert np.array_equal(res["score"], score[:w] + 0.0)
    assert res["new_strat"] == new_strat and res["n_total"] == L.S.shape[0]
    if strat == 4:
        assert res["counters"]["strong"] == cnt["strong"] and res["counters"]["violated"] == cnt["violated"]
        assert res["counters"]["nb_positive"] == int((L.obj > 0).sum())
        assert res["counters"]["nb_violated"] == int((eig_dev < -1e-15).sum())


# ------------------------------------------------------------------------------------------------------------------- 1
def test_rescore_kernel_is_the_oracle_bit_for_bit_on_mixed_sizes(oracle, golden_boxqp):
    """exact_rescore_kernel through a round whose band is the whole list: a shuffled random list of 4099 candidates (not a
    multiple of 64, more than the kernel's grid) of sizes 2..5 on spar040-030-1, strategy 2, head = list -- every returned score
    is the oracle's obj_improve"""
    from sdpcutsel_via_nn_amd import _capi
    g, t = golden_boxqp, "spar040_030_1_d5_"
    n, Q, vv = int(g[t + "nb_vars"]), np.asarray(g[t + "Q_arr"], dtype=np.float64), g[t + "rnd_vars"]
    rng = np.random.default_rng(2)
    N = 4099
    ks = np.ascontiguousarray(rng.integers(2, 6, N), dtype=np.int32)      # ids cross the size classes in random order
    S = np.full((N, 5), -1, dtype=np.int32)
    for i in range(N):
        S[i, :ks[i]] = np.sort(rng.choice(n, int(ks[i]), replace=False))
    assert set(np.unique(ks).tolist()) == {2, 3, 4, 5} and N % 64 != 0 and min(np.bincount(ks)[2:]) > 900
    want = _obj_exact(oracle, S, ks, n, vv, Q)
    sc = _scorer(n, Q, S, ks)
    try:
        sc.set_point(vv)
        res = sc.select_round(2, S.shape[0])
        assert sc.get_stat(_capi.STAT_EXACT_HEAD) == 1
        got = np.empty(S.shape[0])
        got[res["idx"]] = res["score"]
        assert sorted(res["idx"].tolist()) == list(range(S.shape[0]))
        assert np.array_equal(got, want + 0.0), float(np.abs(got - want).max())
        # the twin it is defined by: score_simple_kernel on the same list
        sc.set_option(_capi.OPT_KERNEL, _capi.KERNEL_SIMPLE)
        sc.set_point(vv)
        sc.score(_capi.NN)
        assert np.array_equal(sc.get_scores(eig=False)[1], want)
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("which,sel", [("small", 105), ("big", 5000)])
def test_strategy_2_head_and_scores_are_the_oracles_bits(oracle, request, which, sel):
    from sdpcutsel_via_nn_amd import _capi
    L = request.getfixturevalue(which)
    sc = _scorer(L.n, L.Q, L.S, L.ks, exact=False)
    try:
        sc.set_point(L.vv)
        off = sc.select_round(2, sel)
        obj_fast = sc.get_scores(eig=False)[1]
        assert sc.get_stat(_capi.STAT_EXACT_HEAD) == 0
        assert not np.array_equal(off["score"], np.sort(L.obj)[::-1][:sel])      # today's scores are not the oracle's bits
        sc.set_option(_capi.OPT_EXACT_HEAD, 1)
        sc.set_point(L.vv)
        res = sc.select_round(2, sel)
        assert sc.get_stat(_capi.STAT_EXACT_HEAD) == 1 and sc.get_stat(_capi.STAT_EXACT_GAVE_UP) == 0
        _check_head(oracle, sc, L, 2, sel, res, None)
        assert np.array_equal(sc.get_scores(eig=False)[1], obj_fast)              # d_obj is not written back
        assert sc.get_stat(_capi.STAT_SELECT_FALLBACKS) == 0
        # sdpcut_rank on the scores of the round: the same head
        idx, score, n_total, new_strat, _ = sc.rank(2, 0, max_out=sel)
        assert sc.get_stat(_capi.STAT_EXACT_HEAD) == 1
        assert np.array_equal(idx, res["idx"]) and np.array_equal(score, res["score"]) and n_total == L.S.shape[0]
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("which,regime", [("small", "strong"), ("small", "all"), ("big", "strong"), ("big", "all")])
def test_strategy_4_both_regimes(oracle, request, which, regime):
    from sdpcutsel_via_nn_amd import _capi
    L = request.getfixturevalue(which)
    sc = _scorer(L.n, L.Q, L.S, L.ks)
    try:
        sc.set_point(L.vv)
        sc.score(_capi.EIG | _capi.NN)
        eig_dev = sc.get_scores(obj=False)[0]
        n_strong = int(((L.obj > 0) & (eig_dev < -1e-15)).sum())
        cap_max = 105 if which == "small" else 5000
        assert n_strong >= 8, n_strong
        sel = min(cap_max, n_strong // 2) if regime == "strong" else min(L.S.shape[0], max(n_strong + 50, cap_max))
        if regime == "all":
            assert sel > n_strong and sel <= 7282
        res = sc.round_csr(4, sel, copy=True)
        assert sc.get_stat(_capi.STAT_EXACT_HEAD) == 1 and sc.get_stat(_capi.STAT_EXACT_GAVE_UP) == 0
        _check_head(oracle, sc, L, 4, sel, res, eig_dev)
        assert res["counters"]["strong"] == (sel if regime == "strong" else n_strong)
        # the CSR block is the rows of THAT head
        lam, coef, rhs, cols, ks = sc.cut_rows(res["idx"])
        keep = np.flatnonzero(lam < -1e-15)
        assert np.array_equal(res["row_entry"], keep.astype(np.int32))
        assert np.array_equal(res["rhs"], rhs[keep]) and np.array_equal(res["lam"], lam)
        for r, e in enumerate(keep[:200]):
            ln = int(ks[e]) * (int(ks[e]) + 3) // 2
            a, b = int(res["indptr"][r]), int(res["indptr"][r + 1])
            assert b - a == ln and np.array_equal(res["values"][a:b], coef[e, :ln]) and np.array_equal(res["indices"][a:b], cols[e, :ln])
        # the padded form of the same round
        res2 = sc.select_round(4, sel)
        assert np.array_equal(res2["idx"], res["idx"]) and np.array_equal(res2["score"], res["score"])
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------------------------------- 4
def test_the_admitted_round_is_the_recorded_one_with_the_option_on():
    """rounds 1-3 of the recorded spar125-075-2 dim-3 combined trajectory (132 145 candidates, head 5000).  Option on: every head is
    the recorded one position by position, round 2 included, and the scores that are not -lambda_min are the recorded bits.
    Option off: round 2 still differs in exactly the two admitted pairs (the default did not move)."""
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import _capi
    g = np.load(os.path.join(GOLDEN, "rounds_spar125_075_2_d3_s4.npz"))
    inst = _instance(str(g["name"]))
    sel = int(g["sel_size"])
    sc = pkg.Scorer(0)
    try:
        sc.set_builtin_networks(3)
        sc.set_instance(inst["nb_vars"], inst["Q_arr"])
        assert sc.set_candidates_cover(inst["adj"], 3) == 132145
        for exact in (1, 0):
            sc.set_option(_capi.OPT_EXACT_HEAD, exact)
            for r in (1, 2, 3):
                p = "r%02d_" % r
                strat = int(g[p + "strat"])
                sc.set_point(g[p + "vars"])
                res = sc.select_round(strat, sel)
                ref_ids, ref_score = g[p + "ids"].astype(np.int64), g[p + "score"]
                assert res["new_strat"] == int(g[p + "new_strat"]) and res["n_total"] == int(g[p + "list_len"])
                if not exact:
                    if r == 2:
                        d = np.flatnonzero(res["idx"] != ref_ids)
                        assert sorted(ref_ids[d].tolist()) == sorted([41980, 110560, 98522, 87399]), ref_ids[d]
                    continue
                assert np.array_equal(res["idx"], ref_ids), (r, np.flatnonzero(res["idx"] != ref_ids)[:6])
                if strat in (2, 4) and sc.get_stat(_capi.STAT_EXACT_HEAD) == 0:
                    # a structured LP vertex (masses of equal scores at the threshold) may give up: the head is then the default's,
                    # which is the recorded one in these rounds, and nothing is claimed about the bits of its scores
                    assert sc.get_stat(_capi.STAT_EXACT_GAVE_UP) >= 1 and r != 2
                    continue
                if strat in (2, 4):
                    eig_dev = sc.get_scores(obj=False)[0] if strat == 4 else None
                    is_eig = np.zeros(ref_ids.shape[0], dtype=bool) if eig_dev is None else np.abs(ref_score + eig_dev[ref_ids]) <= 1e-12
                    assert np.array_equal(res["score"][~is_eig], ref_score[~is_eig]), r
                    assert (~is_eig).sum() > 0 or r != 2
            if exact:
                assert sc.get_stat(_capi.STAT_SELECT_FALLBACKS) == 0
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------------------------------- 5
def test_zero_band_decides_the_class_by_the_exact_sign(oracle, small):
    """A violated candidate whose exact obj_improve is below 1e-13 max_elem: obj_improve is linear in every X entry of the
    candidate's own slice (X is no input of the network), so a bisection on ONE entry of the point with the CPU oracle drives it
    there (fixed seed, bounded budget; skips if the budget runs out).  The fast score cannot decide that sign; head and counters
    must follow the exact one."""
    from sdpcutsel_via_nn_amd import _capi
    L = small
    n, Q = L.n, L.Q
    nl = n * (n + 1) // 2
    sc = _scorer(n, Q, L.S, L.ks)
    try:
        sc.set_point(L.vv)
        sc.score(_capi.EIG)
        eig0 = sc.get_scores(obj=False)[0]
        cand = [c for c in np.argsort(np.abs(L.obj)) if eig0[c] < -1e-3][:2]
        found = None
        for c in cand:
            s = L.S[c, :3]
            pos = oracle.triu_positions(s, n)
            q = Q[pos]
            j = int(np.argmax(np.abs(q)))
            if q[j] == 0.0:
                continue
            me = 3.0 * np.abs(q).max()
            vv = L.vv.copy()

            def f(t):
                vv[pos[j]] = t
                return float(oracle.opt_score_batch(3, s[None, :], n, vv, Q)[0])
            t0 = L.vv[pos[j]]
            slope = -q[j]          # d obj / d X_j = -(q_j / max_elem) max_elem
            lo, hi = t0 + f(t0) / (-slope) - 1e-6, t0 + f(t0) / (-slope) + 1e-6
            flo, fhi = f(lo), f(hi)
            if flo * fhi > 0:
                continue
            for _ in range(200):
                mid = 0.5 * (lo + hi)
                fm = f(mid)
                if abs(fm) < 1e-13 * me and fm != 0.0:
                    found = (c, mid, fm)
                    break
                if fm * flo > 0:
                    lo, flo = mid, fm
                else:
                    hi, fhi = mid, fm
            if found:
                vv[pos[j]] = found[1]
                break
        if not found:
            pytest.skip("the bisection found no candidate with |obj_exact| < 1e-13 max_elem within its budget")
        obj = _obj_exact(oracle, L.S, L.ks, n, vv, Q)
        assert 0.0 < abs(obj[found[0]]) < 1e-13 * 3.0 * np.abs(Q).max() * 5
        sc.set_point(vv)
        sc.score(_capi.EIG | _capi.NN)
        eig_dev, obj_fast = sc.get_scores()
        assert eig_dev[found[0]] < -1e-15
        L2 = _List.__new__(_List)
        L2.n, L2.Q, L2.S, L2.ks, L2.vv, L2.obj = n, Q, L.S, L.ks, vv, obj
        n_strong = int(((obj > 0) & (eig_dev < -1e-15)).sum())
        for sel in (max(2, n_strong // 2), min(1051, n_strong + 40)):
            res = sc.select_round(4, sel)
            assert sc.get_stat(_capi.STAT_EXACT_HEAD) == 1
            _check_head(oracle, sc, L2, 4, sel, res, eig_dev)
        assert np.array_equal(sc.get_scores(eig=False)[1], obj_fast)      # the stand-in values have left d_obj again
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------------------------------- 6
def test_honest_give_up(oracle, small):
    """20 000 copies of one triple, head 100, strategy 2: no band of <= 8192 entries separates the threshold.  The call succeeds
    with exactly the option-off result and says so; the next round on a normal list is exact again."""
    from sdpcutsel_via_nn_amd import _capi
    L = small
    S = np.repeat(L.S[:1], 20000, axis=0)
    ks = np.full(20000, 3, dtype=np.int32)
    sc = _scorer(L.n, L.Q, S, ks, exact=False)
    try:
        sc.set_point(L.vv)
        off = sc.select_round(2, 100)
        sc.set_option(_capi.OPT_EXACT_HEAD, 1)
        before = sc.get_stat(_capi.STAT_EXACT_GAVE_UP)
        sc.set_point(L.vv)
        on = sc.select_round(2, 100)
        assert sc.get_stat(_capi.STAT_EXACT_HEAD) == 0 and sc.get_stat(_capi.STAT_EXACT_GAVE_UP) == before + 1
        for key in ("idx", "score", "lam", "coef", "rhs", "ks"):
            assert np.array_equal(on[key], off[key]), key
        assert on["n_total"] == off["n_total"] and on["new_strat"] == off["new_strat"] and on["counters"] == off["counters"]
        sc.set_candidates(L.S, L.ks)
        sc.set_point(L.vv)
        res = sc.select_round(2, 105)
        assert sc.get_stat(_capi.STAT_EXACT_HEAD) == 1 and sc.get_stat(_capi.STAT_EXACT_GAVE_UP) == before + 1
        _check_head(oracle, sc, L, 2, 105, res, None)
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------------------------------- 7
def test_refusals_and_strategies_the_option_ignores(big):
    import torch
    from sdpcutsel_via_nn_amd import _capi
    from sdpcutsel_via_nn_amd._capi import SdpCutError
    L = big
    sc = _scorer(L.n, L.Q, L.S, L.ks)
    try:
        sc.set_point(L.vv)
        with pytest.raises(ValueError, match=EINVAL_TEXT):          # SDPCUT_EINVAL
            sc.select_round(2, 9000)
        rec = torch.zeros(8 + 2 * 64, dtype=torch.int64, device="cuda")
        with pytest.raises(SdpCutError, match="error -4"):          # SDPCUT_ESTATE
            sc.shard_head_device(2, 64, rec.data_ptr())
        on = sc.select_round(1, 5000)
        assert sc.get_stat(_capi.STAT_EXACT_HEAD) == 0
        sc.set_option(_capi.OPT_EXACT_HEAD, 0)
        sc.set_point(L.vv)
        off = sc.select_round(1, 5000)
        for key in ("idx", "score", "lam", "coef", "rhs", "ks"):
            assert np.array_equal(on[key], off[key]), key
        sc.shard_head_device(2, 64, rec.data_ptr())                  # accepted again with the option off
        sc.synchronize()
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------------------------------- 8
def test_drop_in_with_exact_heads():
    """CutSolver(exact_heads=True): same cut counts as the default run; the round-1 head through the drop-in method against the
    published fig. 8 scores, as tests/test_gpu_end_to_end.py checks the default"""
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import _capi, harness
    from sdpcutsel_via_nn_amd.cut_solver import AggArrays
    path = os.path.join(GOLDEN, "instances", "spar020-100-1.in")
    runs = []
    for exact in (False, True):
        cs = pkg.CutSolver(exact_heads=exact)
        bounds, _, _, _, nb_cuts, _, nb_sub = cs.cut_select_algo(path, 3, 0.1, strat=2, nb_rounds_cuts=2)
        runs.append((nb_cuts, nb_sub))
        assert bounds[0] > bounds[1] > bounds[2]
    assert runs[0] == runs[1] and runs[1][0][:2] == [0, 105]
    rows = np.loadtxt(os.path.join(GOLDEN, "fig8_round1.csv"), delimiter=",", skiprows=1)
    inst = harness.parse_boxqp(path)
    lp = harness.boxqp_relaxation(inst)
    lp.solve()
    vv = np.asarray(lp.get_values())
    S, ks, N = _capi.enumerate_cover(inst["adj"], 3)
    cs = pkg.CutSolver(exact_heads=True)
    cs.set_instance(inst["nb_vars"], inst["Q_arr"], AggArrays(S, ks, inst["nb_vars"], inst["Q_arr"]), dim=3, my_prob=lp)
    rl = cs._sel_eigcut_by_ordering_on_measure(2, vv, 1)
    ids, scores = rl.ids(), rl.scores()
    pub_ids, pub_score = rows[:, 1].astype(np.int64), rows[:, 4]
    w = min(len(ids), pub_score.shape[0])
    assert np.allclose(scores[:w], pub_score[:w], rtol=1e-9, atol=1e-10)
    by_id = np.zeros(N)
    by_id[pub_ids] = pub_score
    assert np.all(np.abs(by_id[ids[:w]] - pub_score[:w]) <= 1e-9 * np.maximum(1.0, np.abs(pub_score[:w])))   # same order up to ties
