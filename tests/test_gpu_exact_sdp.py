"""Exact-SDP optimality measure on the device (SDPCUT_SDP, SDPCUT_OPT_EXACT_SDP: strategies 3 and -1) against the numpy twin of its
solver (sdpcutsel_via_nn_amd/exact_sdp.py), the independent certificate check and the published MOSEK column
(tests/golden/fig8_round1.csv).  Bounds: a device value and a twin value both bracket p* from below within their own gaps, so they
differ by at most the two gaps; the published column carries MOSEK's tolerance (test_exact_sdp_cpu.PUBLISHED_BOUND)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden_nn
from sdpcutsel_via_nn_amd import _capi, exact_sdp
from test_exact_sdp_cpu import PUBLISHED_BOUND, TAG, cover_inputs, published

pytestmark = pytest.mark.gpu
MIXED = "spar040_030_1_d5"
PATH = os.path.join(GOLDEN, "instances", "spar020-100-1.in")


def _scorer(z, tag, networks=False, exact_sdp_opt=False):
    import sdpcutsel_via_nn_amd as pkg
    sc = pkg.Scorer(0)
    if networks:
        sc.set_builtin_networks(5)
    if exact_sdp_opt:
        sc.set_option(_capi.OPT_EXACT_SDP, 1)
    sc.set_instance(int(z[tag + "_nb_vars"]), z[tag + "_Q_arr"])
    sc.set_candidates(z[tag + "_set_inds"], z[tag + "_k"])
    sc.set_point(z[tag + "_mck_vars"])
    return sc


def _twin_measure(z, tag):
    N = z[tag + "_k"].shape[0]
    meas, gap = np.zeros(N), np.zeros(N)
    for k, (m, inp, negSM, me) in cover_inputs(z, tag, "mck").items():
        r = exact_sdp.solve(k, inp)
        meas[m], gap[m] = negSM + r["value"] * me, r["gap"] * me
    return meas, gap


@pytest.fixture(scope="module")
def fig8(golden_boxqp):
    """spar020-100-1, dim 3, McCormick point: score(EIG | NN), then score(SDP); every array fetched once"""
    sc = _scorer(golden_boxqp, TAG, networks=True, exact_sdp_opt=True)
    sc.score(_capi.EIG | _capi.NN)
    eig0, obj0 = sc.get_scores()
    scored0 = sc.get_stat(_capi.STAT_SCORED)
    sc.score(_capi.SDP)
    eig1, obj1 = sc.get_scores()
    sdp, gap = sc.get_sdp_scores()
    return dict(sc=sc, eig0=eig0, obj0=obj0, eig1=eig1, obj1=obj1, sdp=sdp, gap=gap, scored0=scored0, scored1=sc.get_stat(_capi.STAT_SCORED),
                unconverged=sc.get_stat(_capi.STAT_SDP_UNCONVERGED), max_elem=golden_boxqp[TAG + "_max_elem"])


@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_sdp_batch_against_twin_and_certificate(k):
    import sdpcutsel_via_nn_amd as pkg
    inp = golden_nn(k)["inputs"]
    assert inp.shape[0] == 4096
    sc = pkg.Scorer(0)                                   # nothing but the handle
    r = sc.sdp_batch(k, inp, want_certificate=True)
    unconverged = sc.get_stat(_capi.STAT_SDP_UNCONVERGED)
    v2, g2 = sc.sdp_batch(k, inp[:100])                  # without the certificate: the same values
    sc.close()
    t = exact_sdp.solve(k, inp)
    x, C, _ = exact_sdp.unpack(k, inp)
    c = exact_sdp.certificate_check(C, np.maximum(x - x * x, 0.0), r["lam"], r["Y"])
    print("k = %d: max |device - twin| %.3e, device gap max %.3e, iterations max %d (twin %d), certificate worst %.3f units"
          % (k, np.abs(r["value"] - t["value"]).max(), r["gap"].max(), r["iters"].max(), t["iters"].max(), c["worst_units"]))
    assert np.all(np.abs(r["value"] - t["value"]) <= r["gap"] + t["gap"] + 1e-15)
    assert c["ok"].all()
    assert unconverged == 0 and r["iters"].max() < exact_sdp.ITER_CAP
    assert np.all(r["gap"] >= 0) and np.all(r["gap"] <= exact_sdp.GAP_TOL * np.maximum(1.0, np.abs(r["value"])))
    assert np.array_equal(v2, r["value"][:100]) and np.array_equal(g2, r["gap"][:100])


def test_score_sdp_against_published_column(fig8):
    exact, sel = published()
    rel = np.abs(fig8["sdp"] - exact) / np.maximum(1.0, np.abs(exact))
    print("worst |device - published| %.3e absolute, %.3e relative" % (np.abs(fig8["sdp"] - exact).max(), rel.max()))
    assert fig8["sdp"].shape == (1051,) and rel.max() <= PUBLISHED_BOUND
    # gap <= GAP_TOL max(1, |p*|), and |p*| <= (k + 1) / 2 = 2 at k = 3: k(k+1)/2 products of a weight |q| <= 1/k and an |X_ij| <= 1
    assert fig8["unconverged"] == 0 and np.all(fig8["gap"] >= 0) and fig8["gap"].max() <= 2 * exact_sdp.GAP_TOL
    assert set(np.argsort(-fig8["sdp"], kind="stable")[:100].tolist()) == set(np.flatnonzero(sel).tolist())


def test_score_sdp_leaves_the_other_measures_alone(fig8):
    assert fig8["scored0"] == (_capi.EIG | _capi.NN) and fig8["scored1"] == (_capi.EIG | _capi.NN | _capi.SDP)
    assert np.array_equal(fig8["eig0"].view(np.int64), fig8["eig1"].view(np.int64))
    assert np.array_equal(fig8["obj0"].view(np.int64), fig8["obj1"].view(np.int64))


def test_score_sdp_mixed_cover_against_twin(golden_boxqp):
    z = golden_boxqp
    assert sorted(np.unique(z[MIXED + "_k"]).tolist()) == [2, 3, 4, 5]
    sc = _scorer(z, MIXED)                               # no networks
    with pytest.raises(_capi.SdpCutError):
        sc.get_sdp_scores()                              # not scored yet
    sc.score(_capi.SDP)
    sdp, gap = sc.get_sdp_scores()
    assert sc.get_stat(_capi.STAT_SCORED) == _capi.SDP and sc.get_stat(_capi.STAT_SDP_UNCONVERGED) == 0
    sc.set_point(z[MIXED + "_mck_vars"])                 # a new point clears the bit like the others
    assert sc.get_stat(_capi.STAT_SCORED) == 0
    with pytest.raises(_capi.SdpCutError):
        sc.get_sdp_scores()
    sc.close()
    meas, tgap = _twin_measure(z, MIXED)
    me = z[MIXED + "_max_elem"]
    assert np.all(np.abs(sdp - meas) <= gap * me + tgap + 1e-12 * np.maximum(1.0, np.abs(meas)))


def test_strategy_3_is_refused_without_the_option(golden_boxqp):
    sc = _scorer(golden_boxqp, TAG, networks=True)
    sc.score(_capi.EIG | _capi.NN | _capi.SDP)
    with pytest.raises(ValueError):
        sc.rank(3, 5)
    with pytest.raises(ValueError):
        sc.round_csr(3, 5)
    with pytest.raises(ValueError):
        sc.select_round(3, 5)
    sc.close()


def test_strategy_3_ranks_the_devices_own_scores(fig8, golden_boxqp):
    sc, sdp = fig8["sc"], fig8["sdp"]
    order = np.argsort(-sdp, kind="stable")
    ids, score, total, new_strat, cnt = sc.rank(3, 0)                  # the whole list
    assert total == 1051 and new_strat == 3 and np.array_equal(ids, order) and np.array_equal(score, sdp[order])
    assert cnt["nb_positive"] == int(np.count_nonzero(sdp > 0))
    ids_h, score_h, total_h, _, _ = sc.rank(3, 0, max_out=100)         # a head (radix select)
    assert total_h == 1051 and np.array_equal(ids_h, order[:100]) and np.array_equal(score_h, sdp[order[:100]])
    # the fused calls on a fresh point: they score SDPCUT_SDP themselves, rank, and emit the rows of those ids bit for bit
    vv = golden_boxqp[TAG + "_mck_vars"]
    r = sc.round_csr(3, 105, point=vv, copy=True)
    assert sc.get_stat(_capi.STAT_SCORED) & _capi.SDP
    assert r["n_total"] == 1051 and r["new_strat"] == 3 and np.array_equal(r["idx"], order[:105]) and np.array_equal(r["score"], sdp[order[:105]])
    lam, coef, rhs, cols, ks = sc.cut_rows(r["idx"])
    keep = np.flatnonzero(lam < -1e-15)
    assert np.array_equal(r["row_entry"], keep) and np.array_equal(r["rhs"].view(np.int64), rhs[keep].view(np.int64))
    for c, e in enumerate(keep):
        w = int(ks[e]) * (int(ks[e]) + 3) // 2
        lo, hi = r["indptr"][c], r["indptr"][c + 1]
        assert np.array_equal(r["indices"][lo:hi], cols[e, :w]) and np.array_equal(r["values"][lo:hi].view(np.int64), coef[e, :w].view(np.int64))
    sc.round_csr_begin(3, 105, point=vv)
    r2 = sc.round_csr_end(copy=True)
    assert np.array_equal(r2["idx"], r["idx"]) and np.array_equal(r2["values"].view(np.int64), r["values"].view(np.int64))
    s = sc.select_round(3, 105, point=vv)
    assert np.array_equal(s["idx"], r["idx"]) and s["new_strat"] == 3 and np.array_equal(s["lam"].view(np.int64), lam.view(np.int64))


def test_strategy_3_full_list_and_window():
    """a list longer than the radix select's longest head (16384): the full device sort, and sdpcut_rank_fetch on its result"""
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import synthetic
    wl = synthetic.make_workload(nb_vars=30, k=3, count=20001, seed=11)
    sc = pkg.Scorer(0)
    sc.set_option(_capi.OPT_EXACT_SDP, 1)
    sc.set_instance(30, wl["Q_arr"])
    sc.set_candidates(wl["set_inds"], wl["ks"])
    sc.set_point(wl["vars_values"])
    with pytest.raises(_capi.SdpCutError):
        sc.rank(3, 0)                                    # sdpcut_rank needs the measure scored
    sc.score(_capi.SDP)
    sdp, gap = sc.get_sdp_scores()
    assert sc.get_stat(_capi.STAT_SDP_UNCONVERGED) == 0 and np.all(np.isfinite(sdp)) and np.all(gap >= 0)
    order = np.argsort(-sdp, kind="stable")
    ids, score, total, new_strat, _ = sc.rank(3, 0)
    assert total == 20001 and new_strat == 3 and np.array_equal(ids, order) and np.array_equal(score, sdp[order])
    w_ids, w_sc = sc.rank_fetch(17000, 333)
    assert np.array_equal(w_ids, order[17000:17333]) and np.array_equal(w_sc, sdp[order[17000:17333]])
    sc.close()


def test_option_is_ignored_by_the_other_strategies(golden_boxqp):
    heads = {}
    for on in (False, True):
        sc = _scorer(golden_boxqp, TAG, networks=True, exact_sdp_opt=on)
        for strat in (1, 2, 4):
            r = sc.round_csr(strat, 105, point=golden_boxqp[TAG + "_mck_vars"], copy=True)
            heads[on, strat] = (r["idx"], r["score"], r["new_strat"], r["values"])
        sc.close()
    for strat in (1, 2, 4):
        a, b = heads[False, strat], heads[True, strat]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64)) and a[2] == b[2]
        assert np.array_equal(a[3].view(np.int64), b[3].view(np.int64))


def _mixin_solver(z, tag, **kw):
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd.cut_solver import AggArrays
    n = int(z[tag + "_nb_vars"])
    cs = pkg.CutSolver(**kw)
    cs.set_instance(n, z[tag + "_Q_arr"], AggArrays(z[tag + "_set_inds"], z[tag + "_k"], n, z[tag + "_Q_arr"]), 3)
    return cs


def test_strategy_minus_1_through_the_mixin(fig8, golden_boxqp):
    z = golden_boxqp
    vv = z[TAG + "_mck_vars"]
    with pytest.raises(NotImplementedError):
        _mixin_solver(z, TAG)._sel_eigcut_by_ordering_on_measure(-1, vv, 1, sel_size=100)
    cs = _mixin_solver(z, TAG, exact_sdp=True)
    rank_list, overlap, std_dev_exact, rows = cs._sel_eigcut_by_ordering_on_measure(-1, vv, 1, sel_size=100)
    nn, ex = fig8["obj0"], fig8["sdp"]
    # cut_select_qp.py:687-702 restated, fed with the device arrays
    rl = sorted([(i, nn[i]) for i in range(1051)], key=lambda e: e[1], reverse=True)
    el = sorted([(i, ex[i]) for i in range(1051)], key=lambda e: e[1], reverse=True)
    pos = {c: p for p, (c, _) in enumerate(el)}
    ref_rows, both = [], 0
    for estim_idx, cut in enumerate(rl):
        a, b = (1 if estim_idx < 100 else 0), (1 if pos[cut[0]] < 100 else 0)
        ref_rows.append([1, cut[0], a, b, cut[1], el[pos[cut[0]]][1]])
        both += a and b
    assert rows == ref_rows and overlap == both / 100
    assert std_dev_exact == np.std(np.array([e[1] for e in el[:100]]))
    assert len(rank_list) == 1051 and [e[0] for e in rank_list[0:100]] == [e[0] for e in rl[:100]]
    L = 20 * 21 // 2
    e0 = rank_list[0]
    s0 = [int(v) for v in z[TAG + "_set_inds"][e0[0], :3]]
    assert e0[1] == rl[0][1] and e0[2] == tuple(vv[L + i] for i in s0)
    # against the published flags: the exact selection is the published one, and so is the overlap with the estimated selection
    csv = np.loadtxt(os.path.join(GOLDEN, "fig8_round1.csv"), delimiter=",", skiprows=1)
    ids = csv[:, 1].astype(int)
    sel_estim, sel_exact = np.zeros(1051, dtype=bool), np.zeros(1051, dtype=bool)
    sel_estim[ids], sel_exact[ids] = csv[:, 2] > 0, csv[:, 3] > 0
    mine_exact = np.zeros(1051, dtype=bool)
    mine_exact[[r[1] for r in rows if r[3]]] = True
    assert np.array_equal(mine_exact, sel_exact)
    # (the published estimated head is the golden strategy-2 head of this point; its 100th and 101st scores lie 0.03 apart)
    assert np.array_equal(np.sort([r[1] for r in rows if r[2]]), np.flatnonzero(sel_estim))
    assert overlap == np.count_nonzero(sel_estim & sel_exact) / 100
    # strategy 3 through the mixin: the layout of strategy 2 on the exact measure
    rl3 = cs._sel_eigcut_by_ordering_on_measure(3, vv, 1)
    order = np.argsort(-ex, kind="stable")
    assert len(rl3) == 1051 and [e[0] for e in rl3[0:50]] == order[:50].tolist() and rl3[0][1] == ex[order[0]]
    assert len(rl3[0]) == 4 and rl3[0][2] == tuple(vv[L + int(i)] for i in z[TAG + "_set_inds"][order[0], :3])


def test_cut_select_algo_strategy_3():
    import sdpcutsel_via_nn_amd as pkg
    with pytest.raises(AssertionError):
        pkg.CutSolver().cut_select_algo(PATH, 3, 0.1, strat=3, nb_rounds_cuts=3)
    bounds, _, _, _, nb_sdp, _, n_cand = pkg.CutSolver(exact_sdp=True).cut_select_algo(PATH, 3, 0.1, strat=3, nb_rounds_cuts=3)
    assert n_cand == 1051 and len(bounds) == 4
    assert all(b1 <= b0 + 1e-9 * abs(b0) for b0, b1 in zip(bounds, bounds[1:])) and bounds[-1] < bounds[0]
    assert nb_sdp[0] == 0 and all(0 <= c <= 105 for c in nb_sdp[1:])


def test_cut_select_algo_figure_8():
    import sdpcutsel_via_nn_amd as pkg
    gap_closed, stats, stds, cuts = pkg.CutSolver(exact_sdp=True).cut_select_algo(PATH, 3, 0.1, strat=-1, nb_rounds_cuts=2, plots=True, sol=706.5)
    assert len(gap_closed) == 3 and gap_closed[0] == 0 and 0 < gap_closed[1] <= gap_closed[2] < 1
    assert len(stats) == len(stds) == 2 and all(0 <= s <= 1 for s in stats) and len(cuts) == 2 * 1051
    exact, _ = published()
    first = np.array([c[5] for c in cuts[:1051]])
    ids = np.array([c[1] for c in cuts[:1051]])
    # round 1 of this loop is the published round: HiGHS and CPLEX may sit on different McCormick vertices, so only report
    print("round 1 of the loop against the published column: worst |delta| %.3e" % np.abs(first - exact[ids]).max())
