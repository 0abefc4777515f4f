"""Diverse cut selection, host side: the numpy twin of the walk (sdpcutsel_via_nn_amd/diversity.py) against brute force on dense
rows, the invariants checker, and the refusals of the Python layer that are decided before a device is touched."""
import types

import numpy as np
import pytest

from sdpcutsel_via_nn_amd import _capi, diversity
from sdpcutsel_via_nn_amd.cut_solver import CutSolver

N_VARS = 12      # few variables: most pairs of candidates share some


def random_pool(P, k, seed, n=N_VARS, duplicates=True):
    """P candidates of size k (k = 0: mixed 2..5) with eigen-cut-like rows [2 v0 v_i | v_i v_j (x 2 off the diagonal)]
    -> (set_inds [P, 5], ks [P], coef [P, 20])"""
    rng = np.random.default_rng(seed)
    S = np.full((P, 5), -1, dtype=np.int32)
    ks = np.zeros(P, dtype=np.int32)
    C = np.zeros((P, 20))
    for t in range(P):
        kk = k if k else int(rng.integers(2, 6))
        ks[t] = kk
        S[t, :kk] = np.sort(rng.choice(n, kk, replace=False))
        v = rng.standard_normal(kk + 1)
        v /= np.linalg.norm(v)
        row = [2 * v[0] * v[1 + a] for a in range(kk)]
        row += [(v[1 + a] * v[1 + b]) * (1 if a == b else 2) for a in range(kk) for b in range(a, kk)]
        C[t, :len(row)] = row
    if duplicates and P >= 4:      # a list drawn with replacement holds a candidate twice
        for src, dst in ((0, P // 2), (1, P - 1)):
            S[dst], ks[dst], C[dst] = S[src], ks[src], C[src]
    return S, ks, C


def dense_rows(S, ks, C, n=N_VARS):
    """the rows on their LP columns [L + i for i in set_inds] + Xarr_inds as a dense [P, L + n] matrix"""
    L = n * (n + 1) // 2
    A = np.zeros((ks.shape[0], L + n))
    for t in range(ks.shape[0]):
        k = int(ks[t])
        s = [int(v) for v in S[t, :k]]
        cols = [L + i for i in s] + [n * s[a] - s[a] * (s[a] + 1) // 2 + s[b] for a in range(k) for b in range(a, k)]
        A[t, cols] = C[t, :len(cols)]
    return A


def brute_cosines(A):
    nr = np.linalg.norm(A, axis=1)
    return (A @ A.T) / (nr[:, None] * nr[None, :])


def brute_walk(cos, eligible, quota, mp):
    keep = np.zeros(eligible.shape[0], dtype=bool)
    acc = []
    for t in range(eligible.shape[0]):
        if len(acc) >= quota:
            break
        if not eligible[t]:
            continue
        if mp < 1.0 and any(abs(cos[t, s]) > mp for s in acc):
            continue
        keep[t] = True
        acc.append(t)
    return keep


SIZES = [1, 2, 63, 64, 65, 300]


@pytest.mark.parametrize("k", [2, 3, 4, 5, 0])
@pytest.mark.parametrize("P", SIZES)
def test_twin_against_brute_force(k, P):
    S, ks, C = random_pool(P, k, seed=100 * P + k)
    cos = diversity.pair_cosines(S, ks, C)
    ref = brute_cosines(dense_rows(S, ks, C))
    err = np.abs(cos - ref).max()
    print("P %d k %d max |cos - brute| %.2e" % (P, k, err))
    assert err <= 1e-14
    rng = np.random.default_rng(P + k)
    eligible = rng.uniform(size=P) < 0.8
    for mp in (0.1, 0.5, 0.9, 1.0):
        # (random rows: no pair near a threshold, so the product form and the quotient form decide alike; duplicates have cos = 1)
        if mp < 1.0:
            assert diversity.undecided_pairs(S, ks, C, eligible, mp, 1e-12).shape[0] == 0
        for quota in (1, 7, P):
            keep, info = diversity.greedy_filter(S, ks, C, eligible, quota, mp, return_info=True)
            want = brute_walk(ref, eligible, quota, mp)
            assert np.array_equal(keep, want), (mp, quota)
            assert info["pool"] == P and info["examined"] == int(keep.sum()) + info["skipped_nonviolated"] + info["rejected_parallel"]
            if keep.sum() < quota:
                assert info["examined"] == P
            else:
                assert info["examined"] == int(np.flatnonzero(keep)[-1]) + 1
            assert diversity.check_walk(S, ks, C, eligible, quota, mp, keep, examined=info["examined"])


def test_duplicates_are_parallel_but_kept_without_a_filter():
    S, ks, C = random_pool(64, 3, seed=5)
    el = np.ones(64, dtype=bool)
    cos = diversity.pair_cosines(S, ks, C)
    assert abs(cos[32, 0] - 1.0) <= 4e-16 and abs(cos[63, 1] - 1.0) <= 4e-16
    assert not diversity.greedy_filter(S, ks, C, el, 64, 0.999)[32]
    # max_parallel = 1 makes no comparison: a computed cosine of 1 + 1 ulp must not reject anything
    assert diversity.greedy_filter(S, ks, C, el, 64, 1.0).all()


def test_eligibility():
    S, ks, C = random_pool(10, 3, seed=2, duplicates=False)
    lam = np.full(10, -0.1)
    lam[3] = -1e-15        # not below the threshold
    lam[4] = 0.2
    C[5] = 0.0             # a zero row
    el = diversity.eligible_rows(lam, ks, C)
    assert el.tolist() == [True, True, True, False, False, False, True, True, True, True]
    keep = diversity.greedy_filter(S, ks, C, el, 10, 1.0)
    assert np.array_equal(keep, el)


def test_check_walk_catches_corruption():
    S, ks, C = random_pool(300, 0, seed=11)
    el = np.random.default_rng(3).uniform(size=300) < 0.9
    for mp in (0.1, 0.3):
        keep, info = diversity.greedy_filter(S, ks, C, el, 40, mp, return_info=True)
        assert 2 <= keep.sum() and info["rejected_parallel"] > 0
        assert diversity.check_walk(S, ks, C, el, 40, mp, keep, margin=1e-12, examined=info["examined"])
        acc = np.flatnonzero(keep)
        # an accepted entry flipped to rejected: nothing accepted in front of it is parallel to it
        bad = keep.copy()
        bad[acc[0]] = False
        with pytest.raises(AssertionError):
            diversity.check_walk(S, ks, C, el, 40, mp, bad, margin=1e-12)
        # a rejected entry flipped to accepted: it is parallel to an accepted one (or the quota overflows)
        rej = np.flatnonzero(el & ~keep & (np.arange(300) < acc[-1]))
        bad = keep.copy()
        bad[rej[0]] = True
        with pytest.raises(AssertionError):
            diversity.check_walk(S, ks, C, el, 40, mp, bad, margin=1e-12)
        # a non-eligible entry accepted
        bad = keep.copy()
        bad[np.flatnonzero(~el)[0]] = True
        with pytest.raises(AssertionError):
            diversity.check_walk(S, ks, C, el, 41, mp, bad, margin=1e-12)
    # the quota not reached although an eligible, unopposed entry is left
    keep = diversity.greedy_filter(S, ks, C, el, 300, 0.5)
    bad = keep.copy()
    bad[np.flatnonzero(keep)[-1]] = False
    with pytest.raises(AssertionError):
        diversity.check_walk(S, ks, C, el, 300, 0.5, bad, margin=1e-12)
    with pytest.raises(AssertionError):      # ... or the walk claims to have stopped early
        diversity.check_walk(S, ks, C, el, 300, 0.5, keep, examined=299)


def test_monotonicity():
    S, ks, C = random_pool(300, 3, seed=21)
    el = np.random.default_rng(4).uniform(size=300) < 0.7
    for quota in (1, 25, 300):
        keep = diversity.greedy_filter(S, ks, C, el, quota, 1.0)
        assert np.array_equal(np.flatnonzero(keep), np.flatnonzero(el)[:quota])
    cos = np.abs(diversity.pair_cosines(S, ks, C))
    for mp in (0.0, 0.1, 0.5, 0.9):
        keep = diversity.greedy_filter(S, ks, C, el, 300, mp)
        acc = np.flatnonzero(keep)
        for i, t in enumerate(acc):      # no accepted entry has an accepted conflicting predecessor
            assert not (cos[t, acc[:i]] > mp).any()
        assert keep[np.flatnonzero(el)[0]]      # the best eligible entry is always taken


def test_refusals_before_a_device_is_touched():
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            _capi.check_diverse_args(bad, 10)
        with pytest.raises(ValueError):
            diversity.greedy_filter(*random_pool(4, 3, 1), np.ones(4, bool), 2, bad)
    with pytest.raises(ValueError):
        _capi.check_diverse_args(0.5, 0)
    with pytest.raises(ValueError):
        _capi.check_diverse_args(0.5, 10, pool_size=9)
    with pytest.raises(ValueError):
        _capi.check_diverse_args(0.5, 10, pool_size=_capi.DIVERSE_MAX_POOL + 1)
    for strat in (0, 3, -1, 5, 104):
        with pytest.raises(ValueError):
            _capi.check_diverse_args(0.5, 10, strat=strat)
    assert _capi.check_diverse_args(0.5, 10, strat=4) == (0.5, 10, 40)
    assert _capi.check_diverse_args(1, 5000) == (1.0, 5000, _capi.DIVERSE_MAX_POOL)
    # the Scorer's methods decide these before they look at their handle
    nobody = types.SimpleNamespace()
    with pytest.raises(ValueError):
        _capi.Scorer.round_csr_diverse(nobody, None, 3, 10, 0.5)
    with pytest.raises(ValueError):
        _capi.Scorer.round_csr_diverse(nobody, None, 1, 10, 0.5, pool_size=5)
    with pytest.raises(ValueError):
        _capi.Scorer.filter_parallel(nobody, [0, 1], 0, 0.5)
    with pytest.raises(ValueError):
        _capi.Scorer.filter_parallel(nobody, np.zeros(_capi.DIVERSE_MAX_POOL + 1, dtype=np.int64), 1, 0.5)
    # cut_select_algo: the filter exists for the ranked strategies only
    for strat in (0, 5):
        with pytest.raises(AssertionError):
            CutSolver().cut_select_algo("no such file", 3, 0.1, strat=strat, max_parallel=0.5)
    with pytest.raises(AssertionError):
        CutSolver().cut_select_algo("no such file", 3, 0.1, strat=1, max_parallel=1.5)
