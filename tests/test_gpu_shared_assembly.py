"""The ordered CSR assembly shared by the plain, the batched and the multi-cut round (csrc/rows_dev.h: csr_lookback): the
look-back across workgroup boundaries when the workgroups keep different numbers of rows.

Input: spar020-100-1 (n = 20) with the 2-, 3- and 4-subsets interleaved (all 190 pairs, 300 each of the others), ranked by
strategy 2 -- the estimated objective improvement, so the head holds entries without a violated eigenvalue between those with
one.  Heads: 193 = 3 x 64 + 1 entries for the plain and the batched assembly (64 entries per workgroup), 97 = 3 x 32 + 1 for
the multi-cut one (32 per workgroup): the last workgroup has one live lane.  At the points used (random_mccormick_point, seeds 7,
8, 9) each of the first three workgroups keeps some entries and skips others (checked with the CPU oracle when the case was
chosen: seed 7 keeps 42, 23, 47 of 64 and 25, 17, 7 of 32); every test asserts that again on what the device returns.

Everything is derived from the returned block itself and is exact: row_entry is the ascending list of head positions with
ks > 0 and lam_min < -1e-15 (multi-cut: each repeated min(n_neg, m) times, cut at the quota), indptr the running sum of
k (k + 3) / 2 over those rows, the array lengths (the header's n_rows and nnz) the ends of both, and the indices of a row the LP
columns of its index set."""
import itertools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INST = os.path.join(ROOT, "tests", "golden", "instances", "spar020-100-1.in")
N = 20
L = N * (N + 1) // 2
THR = -1e-15


@pytest.fixture(scope="module")
def scorer():
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import harness
    inst = harness.parse_boxqp(INST)
    parts = [list(itertools.islice(itertools.combinations(range(N), k), 300)) for k in (2, 3, 4)]
    sets = [p[i] for i in range(300) for p in parts if i < len(p)]
    S = np.full((len(sets), 5), -1, dtype=np.int32)
    for i, s in enumerate(sets):
        S[i, :len(s)] = s
    sc = pkg.Scorer(0)
    sc.set_builtin_networks(5)
    sc.set_instance(N, np.asarray(inst["Q_arr"], dtype=np.float64))
    sc.set_candidates(S, np.array([len(s) for s in sets], dtype=np.int32))
    yield sc
    sc.close()


def point(seed):
    from sdpcutsel_via_nn_amd import harness
    return harness.random_mccormick_point(N, np.random.default_rng(seed))


def columns(s):
    """LP columns of the index set s: L + i for the x part, then the packed upper-triangle positions of the pairs, row-major"""
    return [L + int(i) for i in s] + [N * int(a) - int(a) * (int(a) + 1) // 2 + int(b) for n, a in enumerate(s) for b in s[n:]]


def check_block(r, head, tile, rows_per_entry, quota=None):
    """r: a returned round; rows_per_entry [head]: rows every head position offers"""
    ks, lam = r["ks"], r["lam"]
    assert r["idx"].shape[0] == head and ks.shape[0] == head and ks.min() >= 2 and {2, 3} <= set(ks.tolist())
    keep = (ks > 0) & (lam < THR)
    for g in range(3):      # not trivially true: each of the first three workgroups keeps some entries and skips others
        part = keep[g * tile:(g + 1) * tile]
        assert 0 < part.sum() < tile, (g, int(part.sum()))
    assert not np.any(rows_per_entry[~keep]) and np.all(rows_per_entry[keep] >= 1)
    want_entry = np.repeat(np.arange(head, dtype=np.int32), rows_per_entry)
    if quota is not None:
        want_entry = want_entry[:quota]
    k_row = ks[want_entry].astype(np.int64)
    want_indptr = np.concatenate([[0], np.cumsum(k_row * (k_row + 3) // 2)]).astype(np.int32)
    assert r["row_entry"].dtype == np.int32 and np.array_equal(r["row_entry"], want_entry)
    assert r["indptr"].dtype == np.int32 and np.array_equal(r["indptr"], want_indptr)
    assert r["rhs"].shape[0] == want_entry.shape[0]                                      # n_rows of the header
    assert r["indices"].shape[0] == r["values"].shape[0] == int(want_indptr[-1])         # nnz of the header
    want_indices = [c for e in want_entry for c in columns(r["set_inds"][e, :ks[e]])]
    assert np.array_equal(r["indices"], np.array(want_indices, dtype=np.int32))
    return want_entry


def test_plain_round_across_workgroups(scorer):
    r = scorer.round_csr(2, 193, point=point(7), copy=True)
    keep = (r["ks"] > 0) & (r["lam"] < THR)
    check_block(r, 193, 64, keep.astype(np.int64))
    assert {2, 3, 4} <= set(r["ks"].tolist())


def test_batched_round_across_workgroups(scorer):
    pts = np.stack([point(s) for s in (7, 8, 9)])
    n_rows = set()
    for r in scorer.round_csr_points(pts, 2, 193, copy=True):
        keep = (r["ks"] > 0) & (r["lam"] < THR)
        check_block(r, 193, 64, keep.astype(np.int64))
        n_rows.add(int(keep.sum()))
    assert len(n_rows) == 3      # the points keep different numbers of rows: one point's look-back words are not another's


@pytest.mark.parametrize("m", [1, 3])
def test_multi_cut_round_across_workgroups(scorer, m):
    quota = 35
    r = scorer.round_csr_multi(point(7), 2, 97, m, row_quota=quota, copy=True)
    n_neg = r["n_neg"].astype(np.int64)
    assert np.array_equal(n_neg > 0, (r["ks"] > 0) & (r["lam"] < THR))
    offered = np.minimum(n_neg, m)
    # the quota falls inside the second workgroup
    assert offered[:32].sum() < quota < offered[:64].sum()
    rows = check_block(r, 97, 32, offered, quota)
    assert r["quota_hit"] and r["row_cap"] == quota and r["n_used"] == int(rows[-1]) + 1 and 32 < r["n_used"] <= 64
    want_rank = np.concatenate([np.arange(c) for c in offered])[:quota]
    assert np.array_equal(r["row_rank"], want_rank.astype(np.int32))
    if m > 1:
        assert (want_rank > 0).any(), "no entry with a second row in front of the quota"
    # without the quota the walk goes through all four workgroups
    full = scorer.round_csr_multi(point(7), 2, 97, m, row_quota="sets", copy=True)
    assert np.array_equal(full["n_neg"], r["n_neg"])
    check_block(full, 97, 32, offered)
    assert not full["quota_hit"]
