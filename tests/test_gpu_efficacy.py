"""Efficacy ranking (strategy 6, SDPCUT_EFF; csrc/efficacy.hip) on the device against the numpy twin
(sdpcutsel_via_nn_amd/efficacy.py) and against numpy.linalg.eigh.  The lists come from committed fixtures only
(tests/efficacy_cases.py; tests/test_efficacy_cpu.py checks on the CPU what is assumed about them here)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import efficacy_cases as ec  # noqa: E402

ARRAYS = ("idx", "score", "lam", "ks", "set_inds", "row_entry", "indptr", "indices", "values", "rhs")
EIG, NN, EFF = 1, 2, 8


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def scorers():
    """two handles with the shipped networks: the one under test and a fresh one to compare with"""
    import sdpcutsel_via_nn_amd as pkg
    scs = []
    for _ in range(2):
        sc = pkg.Scorer(0)
        sc.set_builtin_networks(5)
        scs.append(sc)
    yield tuple(scs)
    for sc in scs:
        sc.close()


def bind(sc, case, obj=None, w=0.0):
    sc.drop_pending()
    sc.set_instance(case.n, case.Q_arr)
    sc.set_candidates(case.S, case.ks)
    sc.set_objective(obj)
    sc.set_efficacy_weight(w)
    sc.set_point(case.point)


def device_and_twin(sc, case, obj=None, w=0.0):
    """-> (device (eff, objpar, escore), twin (eff, objpar, escore), lam) with the twin fed the device's OWN rows"""
    from sdpcutsel_via_nn_amd import efficacy
    bind(sc, case, obj, w)
    sc.score(EFF)
    dev = sc.get_efficacy()
    lam_dev, _ = sc.get_scores(obj=False)
    lam, coef, rhs, cols, ks = sc.cut_rows(np.arange(case.N))
    assert np.array_equal(ks, case.ks)
    twin = efficacy.measure(lam_dev, coef, cols, ks, obj=obj, w=w)
    return dev, twin, lam_dev


def all_cases():
    return ec.generic_cases() + ec.structured_cases()


# ------------------------------------------------------------------------------------------ 1. the measure against the twin
@pytest.mark.parametrize("ci", range(13))
def test_measure_equals_the_twin_bit_for_bit(scorers, ci):
    """eff, objpar and escore of every candidate equal the twin's on the rows cut_rows returns: the operation order is specified,
    the square root and the division are IEEE.  The structured lists (nothing violated; the McCormick vertex x = 0.5; the
    clustered spectra of tests/spectra_cases.py) are covered by this test only: where lambda_min is multiple a vector of the
    eigenspace is not unique and test 2 has no truth to offer."""
    sc, _ = scorers
    cases = all_cases()
    assert len(cases) == 13
    case = cases[ci]
    for obj, w in ((None, 0.0), (case.obj, 0.1)):
        dev, twin, lam = device_and_twin(sc, case, obj, w)
        for name, d, t in zip(("eff", "objpar", "escore"), dev, twin):
            assert same_bits(d, t), (case.name, name, int(np.flatnonzero(bits(d) != bits(t))[0]))
        assert np.array_equal(dev[0] > 0, lam < -1e-15), case.name                  # the classes separate exactly by sign
        assert not np.any(np.signbit(dev[0][dev[0] == 0.0]))
        if obj is None:
            assert np.all(dev[1] == 0.0) and same_bits(dev[0], dev[2])
        else:
            assert np.all((dev[1] >= 0.0) & (dev[1] <= 1.0))
            if (lam < -1e-15).any():
                assert dev[1].max() > 0.0
        assert sc.get_stat(3) & EFF and sc.get_stat(3) & EIG                        # SDPCUT_STAT_SCORED reports it; EFF implied EIG
    if case.name == "mixed/psd":
        assert np.all(dev[0] <= 0.0) and np.all(lam > 0)


# ------------------------------------------------------------------------------------------ 2. independent truth
@pytest.mark.parametrize("ci", range(7))
def test_efficacy_against_lapack(scorers, ci):
    """-lam / ||coef(v)|| from numpy.linalg.eigh's vector, relative 1e-7, on the generic lists (random interior points, recorded LP
    points after round 2) for candidates whose lambda_min is separated from the next eigenvalue by >= 1e-6 ||A||_F: the
    eigenvector error is a few eps ||A|| / gap ~ 5e-9 and the norm is Lipschitz in v with a constant of about 4."""
    sc, _ = scorers
    case = ec.generic_cases()[ci]
    bind(sc, case)
    sc.score(EFF)
    eff, _, _ = sc.get_efficacy()
    lam, want, sep = ec.truth(case)
    viol = lam < ec.NEG
    use = viol & sep
    assert (viol & ~sep).sum() <= max(0.01 * viol.sum(), 0 if case.N >= 1000 else 1), case.name
    if use.any():
        rel = np.abs(eff[use] - want[use]) / want[use]
        assert rel.max() <= 1e-7, (case.name, float(rel.max()))
    ok = ~viol & (lam > 1e-12)
    assert np.all(eff[ok] <= 0.0)


# ------------------------------------------------------------------------------------------ 3. ranking
@pytest.mark.parametrize("N", [64, 5000, 70000])
def test_ranking_is_the_stable_sort_of_the_devices_escore(scorers, N):
    """rank(6) and rank_device(6): ids and scores of a stable descending sort of the device's own escore, bit for bit, at the
    lengths that take the small, the radix / direct and the strip-cut routes"""
    import torch
    from sdpcutsel_via_nn_amd import efficacy, synthetic
    sc, _ = scorers
    sc.drop_pending()
    n = 200
    Q_arr, _, _ = synthetic.make_instance(n, 7)
    sc.set_instance(n, np.asarray(Q_arr, dtype=np.float64))
    sc.set_candidates_philox(3, N, seed=11)
    obj = np.random.default_rng(5).normal(size=n * (n + 1) // 2 + n)
    sc.set_objective(obj)
    sc.set_efficacy_weight(0.1)
    sc.set_point(ec.random_point(n, 9))
    with pytest.raises(Exception):
        sc.rank(6, 0, 10)                                   # sdpcut_rank needs a preceding score(EFF)
    sc.score(EFF)
    eff, objpar, escore = sc.get_efficacy()
    order = efficacy.ranking(escore)
    nviol = int((eff > 0).sum())
    assert 0 < nviol < N or N == 64
    for max_out in sorted({min(N, 100), min(N, 5000), N}):
        idx, score, total, new_strat, cnt = sc.rank(6, 0, max_out)
        assert (total, new_strat) == (N, 6)
        assert np.array_equal(idx, order[:max_out]) and same_bits(score, escore[order[:max_out]]), (N, max_out)
        assert cnt["nb_positive"] == nviol == cnt["nb_violated"]
    if N > 16384:                                            # the full ranking stays on the device: windows of it
        idx2, sc2 = sc.rank_fetch(N - 777, 777)
        assert np.array_equal(idx2, order[N - 777:]) and same_bits(sc2, escore[order[N - 777:]])
    m = min(N, 3000)
    d_idx = torch.empty(m, dtype=torch.int64, device="cuda")
    d_sc = torch.empty(m, dtype=torch.float64, device="cuda")
    w, total, new_strat, cnt = sc.rank_device(6, 0, m, d_idx.data_ptr(), d_sc.data_ptr())
    sc.synchronize()
    torch.cuda.synchronize()
    assert (w, total, new_strat) == (m, N, 6)
    assert np.array_equal(d_idx.cpu().numpy(), order[:m]) and same_bits(d_sc.cpu().numpy(), escore[order[:m]])


# ------------------------------------------------------------------------------------------ 4. rounds
@pytest.mark.parametrize("ci", [4, 5, 8])
def test_rounds_emit_the_rankings_head_and_the_scored_rows(scorers, ci):
    """round_csr(6), select_round(6), round_view(6) (select_round with a point) and round_csr_begin / _end(6): the head is the
    ranking's, score is escore, the rows are cut_rows of those ids, bit for bit"""
    from sdpcutsel_via_nn_amd import efficacy
    sc, fresh = scorers
    case = all_cases()[ci]
    for sel in (1, 70, case.N):
        dev, twin, lam = device_and_twin(sc, case, case.obj, 0.1)
        escore = dev[2]
        order = efficacy.ranking(escore)[:sel]
        lam_r, coef_r, rhs_r, cols_r, ks_r = sc.cut_rows(order)
        rounds = []
        bind(fresh, case, case.obj, 0.1)
        rounds.append(("round_csr", fresh.round_csr(6, sel, copy=True)))          # scores EIG and EFF itself
        assert fresh.get_stat(3) & EFF
        bind(fresh, case, case.obj, 0.1)
        fresh.round_csr_begin(6, sel)
        with pytest.raises(Exception):
            fresh.set_efficacy_weight(0.2)                                        # refused while a round is pending
        with pytest.raises(Exception):
            fresh.set_objective(None)
        rounds.append(("begin/end", fresh.round_csr_end(copy=True)))
        rounds.append(("round_csr on a scored list", sc.round_csr(6, sel, copy=True)))
        for name, r in rounds:
            assert (r["n_total"], r["new_strat"]) == (case.N, 6), name
            assert np.array_equal(r["idx"], order) and same_bits(r["score"], escore[order]), (case.name, name, sel)
            assert same_bits(r["lam"], lam_r) and np.array_equal(r["ks"], ks_r)
            keep = np.flatnonzero(lam_r < -1e-15)
            assert np.array_equal(r["row_entry"], keep.astype(np.int32))
            assert same_bits(r["rhs"], rhs_r[keep])
            for t, e in enumerate(keep):
                M = int(ks_r[e]) * (int(ks_r[e]) + 3) // 2
                lo, hi = r["indptr"][t], r["indptr"][t + 1]
                assert hi - lo == M and same_bits(r["values"][lo:hi], coef_r[e, :M]) and np.array_equal(r["indices"][lo:hi], cols_r[e, :M])
            assert r["counters"]["nb_positive"] == int((escore > 0).sum())
        for name, r in (("select_round", sc.select_round(6, sel)), ("round_view", fresh.select_round(6, sel, point=case.point))):
            ld = r["coef"].shape[1]
            assert (r["n_total"], r["new_strat"]) == (case.N, 6), name
            assert np.array_equal(r["idx"], order) and same_bits(r["score"], escore[order]), (case.name, name, sel)
            assert same_bits(r["lam"], lam_r) and same_bits(r["rhs"], rhs_r) and same_bits(r["coef"], coef_r[:, :ld]) and np.array_equal(r["ks"], ks_r)


def test_a_list_without_a_violated_candidate_emits_nothing(scorers):
    sc, _ = scorers
    case = {c.name: c for c in ec.structured_cases()}["mixed/psd"]
    bind(sc, case)
    r = sc.round_csr(6, 100, copy=True)
    assert r["idx"].shape[0] == 100 and r["rhs"].shape[0] == 0 and r["indptr"].tolist() == [0] and r["values"].shape[0] == 0
    assert np.all(r["score"] <= 0.0) and r["counters"]["nb_positive"] == 0 and r["counters"]["nb_violated"] == 0
    d = sc.round_csr_diverse(None, 6, 50, 0.5, copy=True)
    assert d["rhs"].shape[0] == 0 and d["idx"].shape[0] == 0
    m = sc.round_csr_multi(None, 6, 50, 5, copy=True)
    assert m["rhs"].shape[0] == 0


# ------------------------------------------------------------------------------------------ 5. diverse and multi-cut rounds
@pytest.mark.parametrize("ci", [4, 5])
def test_diverse_round_on_the_efficacy_ranking(scorers, ci):
    """round_csr_diverse(6, max_parallel = 0.5): the walk of diversity.py over the first pool entries of the strategy-6 ranking --
    compared exactly where no pair's cosine lies within 1e-12 of the threshold, by the walk's invariants otherwise"""
    from sdpcutsel_via_nn_amd import diversity, efficacy
    sc, _ = scorers
    case = all_cases()[ci]
    dev, _, lam = device_and_twin(sc, case)
    order = efficacy.ranking(dev[2])
    sel, pool = 40, 160
    ids = order[:pool]
    lam_r, coef_r, _, _, ks_r = sc.cut_rows(ids)
    el = diversity.eligible_rows(lam_r, ks_r, coef_r)
    d = sc.round_csr_diverse(None, 6, sel, 0.5, pool_size=pool, copy=True)
    assert (d["n_total"], d["new_strat"]) == (case.N, 6)
    at = {int(g): t for t, g in enumerate(ids)}
    keep = np.zeros(pool, dtype=bool)
    keep[[at[int(g)] for g in d["idx"]]] = True
    assert np.array_equal(d["idx"], ids[keep]) and same_bits(d["score"], dev[2][d["idx"]])          # accepted entries in rank order
    cos = diversity.pair_cosines(case.S[ids], ks_r, coef_r)
    diversity.check_walk(case.S[ids], ks_r, coef_r, el, sel, 0.5, keep, margin=1e-12, examined=d["info"]["examined"], cos=cos)
    if diversity.undecided_pairs(case.S[ids], ks_r, coef_r, el, 0.5, 1e-12, cos=cos).shape[0] == 0:
        want = diversity.greedy_filter(case.S[ids], ks_r, coef_r, el, sel, 0.5)
        assert np.array_equal(keep, want)
    assert d["rhs"].shape[0] == d["idx"].shape[0] == int(keep.sum()) > 0


@pytest.mark.parametrize("ci", [4, 5])
def test_multi_cut_round_on_the_efficacy_ranking(scorers, ci):
    """round_csr_multi(6, max_per_set = 5): the head of the strategy-6 ranking, rows checked by multicut.check_rows"""
    from sdpcutsel_via_nn_amd import efficacy, multicut
    sc, _ = scorers
    case = all_cases()[ci]
    dev, _, lam = device_and_twin(sc, case)
    order = efficacy.ranking(dev[2])
    sel = 64
    m = sc.round_csr_multi(None, 6, sel, 5, row_quota="sets", copy=True)
    assert (m["n_total"], m["new_strat"]) == (case.N, 6)
    assert np.array_equal(m["idx"], order[:sel]) and same_bits(m["score"], dev[2][order[:sel]])
    rows = m["rhs"].shape[0]
    assert rows >= int((lam[order[:sel]] < -1e-15).sum()) > 0
    coef = np.zeros((rows, 20))
    for t in range(rows):
        coef[t, :m["indptr"][t + 1] - m["indptr"][t]] = m["values"][m["indptr"][t]:m["indptr"][t + 1]]
    multicut.check_rows(case.S[order[:sel]], case.ks[order[:sel]], case.point, case.n, 5, m["row_entry"], m["row_rank"], m["row_lam"], coef, m["rhs"])
    one = sc.round_csr_multi(None, 6, sel, 1, copy=True)                      # max_per_set = 1 is round_csr
    plain = sc.round_csr(6, sel, copy=True)
    for f in ARRAYS:
        assert np.array_equal(one[f], plain[f]), f


# ------------------------------------------------------------------------------------------ 6. the objective
def test_objective_weight_changes_the_head_and_state_follows(scorers):
    from sdpcutsel_via_nn_amd import _capi, efficacy
    sc, fresh = scorers
    case = ec.generic_cases()[5]          # spar070-050-1 at the LP point its recorded run separated at in round 3
    sel = 50
    heads = {}
    for w, obj in ((0.0, None), (0.1, case.obj)):
        dev, twin, lam = device_and_twin(fresh, case, obj, w)
        r = fresh.round_csr(6, sel, copy=True)
        assert np.array_equal(r["idx"], efficacy.ranking(twin[2])[:sel]) and same_bits(r["score"], twin[2][r["idx"]])
        heads[w] = r
    assert not np.array_equal(heads[0.0]["idx"], heads[0.1]["idx"])          # (chosen on the CPU with the twin: the heads differ here)
    # the same settings reached on a LIVE handle give what a fresh handle gives, byte for byte
    bind(sc, case, None, 0.0)
    sc.score(EFF)
    sc.set_efficacy_weight(0.1)
    assert not sc.get_stat(_capi.STAT_SCORED) & EFF and sc.get_stat(_capi.STAT_SCORED) & EIG      # clears EFF only
    sc.set_objective(case.obj)
    live = sc.round_csr(6, sel, copy=True)
    for f in ARRAYS:
        assert live[f].dtype == heads[0.1][f].dtype and np.array_equal(live[f], heads[0.1][f]), f
    assert same_bits(np.stack(sc.get_efficacy()), np.stack(fresh.get_efficacy()))
    sc.set_objective(None)
    sc.set_efficacy_weight(0.0)
    back = sc.round_csr(6, sel, copy=True)
    for f in ARRAYS:
        assert np.array_equal(back[f], heads[0.0][f]), f
    # set_point invalidates
    sc.set_point(case.point)
    with pytest.raises(_capi.SdpCutError, match="-4|not scored"):
        sc.get_efficacy()
    # argument checks
    for bad in (case.obj[:-1], np.zeros_like(case.obj), np.where(np.arange(case.obj.shape[0]) == 3, np.inf, case.obj)):
        with pytest.raises(ValueError):
            sc.set_objective(bad)
    for w in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            sc.set_efficacy_weight(w)


# ------------------------------------------------------------------------------------------ 7. nothing else moved
def test_other_strategies_do_not_see_the_measure(scorers):
    from sdpcutsel_via_nn_amd import _capi
    sc, _ = scorers
    case = all_cases()[4]

    def snapshot():
        out = {}
        for strat in (1, 2, 4):
            r = sc.round_csr(strat, 80, copy=True)
            out[strat] = [r[f] for f in ARRAYS] + [np.array([r["n_total"], r["new_strat"]] + list(r["counters"].values()))]
        out["scores"] = list(sc.get_scores())
        return out
    bind(sc, case)
    before = snapshot()
    sc.set_objective(case.obj)
    sc.set_efficacy_weight(0.1)
    sc.set_point(case.point)          # (both snapshots start from a point nothing is scored at: a feasibility round reports nb_positive
    sc.score(EFF)                     # of an optimality measure only where one is scored)
    eff0 = sc.get_efficacy()[0]
    after = snapshot()
    for key in before:
        for a, b in zip(before[key], after[key]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), key
    assert sc.get_stat(_capi.STAT_SCORED) & EFF                               # the other strategies' rounds left it scored
    # a node box changes the optimality measures, not this one, and leaves its bit alone
    lb, ub = np.full(case.n, 0.125), np.full(case.n, 0.875)
    sc.set_box(lb, ub)
    assert sc.get_stat(_capi.STAT_SCORED) & EFF
    assert same_bits(sc.get_efficacy()[0], eff0)
    sc.set_point(case.point)
    sc.score(EFF)
    assert same_bits(sc.get_efficacy()[0], eff0)
    boxed = sc.round_csr(6, 80, copy=True)
    sc.clear_box()
    assert sc.get_stat(_capi.STAT_SCORED) & EFF
    plain = sc.round_csr(6, 80, copy=True)
    for f in ARRAYS:
        assert np.array_equal(boxed[f], plain[f]), f


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(scorers):
    from sdpcutsel_via_nn_amd import cut_solver
    sc, _ = scorers
    case = all_cases()[3]
    bind(sc, case)
    pts = np.stack([case.point, case.point])
    with pytest.raises(ValueError, match="strategy 6"):
        sc.round_csr_points(pts, 6, 10)
    lib, h = sc._lib, sc._h
    import ctypes
    e = np.empty((2, case.N))
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.sdpcut_score_points(h, 2, pts.ctypes.data_as(dp), pts.shape[1], EIG | EFF, e.ctypes.data_as(dp), None)
    assert rc == -1 and b"SDPCUT_EFF" in lib.sdpcut_last_error(h)
    sc.set_point(case.point)
    with pytest.raises(ValueError):
        sc.rank(7, 0, 10)
    import torch
    rec = torch.empty(8 + 2 * 64, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="strategy 6"):
        sc.shard_head_device(6, 64, rec.data_ptr())
    path = os.path.join(ec.INST, "q_20_4_25_1.osil")
    with pytest.raises(AssertionError, match="strategy 6"):
        cut_solver.CutSolverQCQP().cut_select_algo(path, 3, strat=6)
