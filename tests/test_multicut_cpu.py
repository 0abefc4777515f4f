"""All violated eigen-cuts of a selected set, the parts that need no device: the numpy twin and checker (multicut.py), the block
layout of the multi-cut round (csrc/round_layout.h: csr_multi_layout), the new names of the C-ABI and the argument checks of the
Python layer."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")
NEG = -1e-15


def point(n, seed):
    from sdpcutsel_via_nn_amd import harness
    return harness.random_mccormick_point(n, np.random.default_rng(seed))


def all_subsets(n):
    sets = [s for k in (2, 3, 4, 5) for s in itertools.combinations(range(n), k)]
    S = np.full((len(sets), 5), -1, dtype=np.int32)
    for i, s in enumerate(sets):
        S[i, :len(s)] = s
    return S, np.array([len(s) for s in sets], dtype=np.int32)


# ------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("seed", [7, 8])
def test_expected_against_a_brute_force_loop(seed):
    """n = 6, all 2-, 3-, 4- and 5-subsets: every row spelled out from numpy.linalg.eigh, one matrix entry at a time"""
    from sdpcutsel_via_nn_amd import multicut
    n = 6
    L = n * (n + 1) // 2
    vv = point(n, seed)
    S, ks = all_subsets(n)
    assert S.shape[0] == 15 + 20 + 15 + 6
    pos = {}
    p = 0
    for i in range(n):
        for j in range(i, n):
            pos[(i, j)] = p
            p += 1
    seen_multi = 0
    for m in (1, 2, 3, 5):
        e = multicut.expected(S, ks, vv, n, m)
        r = 0
        nnz = 0
        for i in range(S.shape[0]):
            s = [int(v) for v in S[i, :ks[i]]]
            k = len(s)
            M = np.empty((k + 1, k + 1))
            M[0, 0] = 1.0
            for a in range(k):
                M[0, a + 1] = M[a + 1, 0] = vv[L + s[a]]
                for b in range(k):
                    M[a + 1, b + 1] = vv[pos[(min(s[a], s[b]), max(s[a], s[b]))]]
            w, V = np.linalg.eigh(M)
            neg = [j for j in range(k + 1) if w[j] < NEG]
            assert e["n_neg"][i] == len(neg) and e["lam_min"][i] == w[0] and e["n_offered"][i] == min(len(neg), m)
            assert len(neg) <= k
            seen_multi += len(neg) >= 2
            cols = [L + v for v in s] + [pos[(s[a], s[b])] for a in range(k) for b in range(a, k)]
            for j in neg[:m]:
                v = V[:, j].copy()
                v[np.abs(v) <= 1e-15] = 0.0
                coef = [2 * v[0] * v[a] for a in range(1, k + 1)]
                coef += [(v[a] * v[b] if a == b else 2 * v[a] * v[b]) for a in range(1, k + 1) for b in range(a, k + 1)]
                assert (e["row_entry"][r], e["row_rank"][r], e["row_lam"][r]) == (i, j, w[j])
                assert e["rhs"][r] == -v[0] * v[0]
                lo, hi = e["indptr"][r], e["indptr"][r + 1]
                assert lo == nnz and hi - lo == len(cols) == k * (k + 3) // 2
                assert e["indices"][lo:hi].tolist() == cols
                assert np.allclose(e["values"][lo:hi], coef, rtol=0, atol=1e-16)
                assert np.array_equal(e["coef"][r, :hi - lo], e["values"][lo:hi]) and not e["coef"][r, hi - lo:].any()
                nnz = hi
                r += 1
        assert r == e["row_entry"].shape[0] == e["rhs"].shape[0] and e["indptr"].shape[0] == r + 1
    assert seen_multi > 0, "no matrix with two violated eigenvalues: the case tests nothing"


def test_walk_against_the_rule_entry_by_entry():
    from sdpcutsel_via_nn_amd import multicut
    rng = np.random.default_rng(3)
    offered = [np.array([2, 0, 3, 1, 0, 5, 2]), np.array([0, 0, 0]), np.array([1]), rng.integers(0, 6, 200)]
    for off in offered:
        total = int(off.sum())
        inside = int(off[:3].sum()) - 1 if off.shape[0] > 2 and off[2] >= 2 else None      # ends inside the third entry
        for q in [1, 2, max(total - 1, 1), max(total, 1), total + 7] + ([inside] if inside else []):
            kept, n_rows, n_used, hit = multicut.walk(off, q)
            want, r, used = [], 0, 0
            for i, o in enumerate(off.tolist()):
                k = 0
                for _ in range(o):
                    if r < q:
                        k += 1
                        r += 1
                if k:
                    used = i + 1
                want.append(k)
            assert kept.tolist() == want and n_rows == r == min(total, q) and n_used == used and hit == (total > q), (off, q)
    kept, n_rows, n_used, hit = multicut.walk(np.array([2, 0, 3, 1]), 4)      # the quota falls inside the third entry
    assert (kept.tolist(), n_rows, n_used, hit) == ([2, 0, 2, 0], 4, 3, True)
    kept, n_rows, n_used, hit = multicut.walk(np.array([2, 0, 3, 1]), 1)
    assert (kept.tolist(), n_rows, n_used, hit) == ([1, 0, 0, 0], 1, 1, True)
    kept, n_rows, n_used, hit = multicut.walk(np.array([2, 0, 3, 1]), 100)
    assert (kept.tolist(), n_rows, n_used, hit) == ([2, 0, 3, 1], 6, 4, False)
    assert multicut.walk(np.zeros(0, dtype=np.int64), 3)[1:] == (0, 0, False)
    with pytest.raises(ValueError):
        multicut.walk(np.array([1]), 0)


def test_check_rows_accepts_the_twin_and_rejects_wrong_answers():
    from sdpcutsel_via_nn_amd import multicut
    n = 6
    vv = point(n, 7)
    S, ks = all_subsets(n)
    e = multicut.expected(S, ks, vv, n, 5)
    args = (S, ks, vv, n, 5)
    assert multicut.check_rows(*args, e["row_entry"], e["row_rank"], e["row_lam"], e["coef"], e["rhs"])
    # the quota: any prefix of the walk is a correct answer to its own quota, and to no larger one
    two = int(np.flatnonzero(e["n_offered"] >= 2)[3])
    q = int(e["n_offered"][:two].sum()) + 1      # ends inside an entry
    t = multicut.apply_walk(e, q)
    assert t["n_rows"] == q and t["quota_hit"] and t["n_used"] == two + 1
    assert multicut.check_rows(*args, t["row_entry"], t["row_rank"], t["row_lam"], t["coef"], t["rhs"], row_quota=q)
    with pytest.raises(AssertionError, match="lacks rows"):
        multicut.check_rows(*args, t["row_entry"], t["row_rank"], t["row_lam"], t["coef"], t["rhs"])
    with pytest.raises(AssertionError, match="lacks rows"):
        multicut.check_rows(*args, t["row_entry"], t["row_rank"], t["row_lam"], t["coef"], t["rhs"], row_quota=q + 1)
    # fewer cuts per set than offered is the answer to a smaller cuts_per_set only
    e2 = multicut.expected(S, ks, vv, n, 2)
    assert multicut.check_rows(S, ks, vv, n, 2, e2["row_entry"], e2["row_rank"], e2["row_lam"], e2["coef"], e2["rhs"])
    if (e["n_offered"] > 2).any():
        with pytest.raises(AssertionError):
            multicut.check_rows(*args, e2["row_entry"], e2["row_rank"], e2["row_lam"], e2["coef"], e2["rhs"])
    r0 = int(np.flatnonzero(e["row_rank"] == 1)[0]) - 1      # rows r0, r0 + 1: ranks 0 and 1 of one entry

    def broken(**change):
        a = {f: e[f].copy() for f in ("row_entry", "row_rank", "row_lam", "coef", "rhs")}
        for f, fn in change.items():
            a[f] = fn(a[f])
        return a["row_entry"], a["row_rank"], a["row_lam"], a["coef"], a["rhs"]

    def swap(a):
        a[[r0, r0 + 1]] = a[[r0 + 1, r0]]
        return a
    # a swapped pair: the two rows of an entry in the wrong order (eigenvalue, coefficients and rhs travel together)
    with pytest.raises(AssertionError):
        multicut.check_rows(*args, *broken(row_lam=swap, coef=swap, rhs=swap))
    # a missing row
    drop = lambda a: np.delete(a, r0 + 1, axis=0)
    with pytest.raises(AssertionError, match="lacks rows"):
        multicut.check_rows(*args, *broken(row_entry=drop, row_rank=drop, row_lam=drop, coef=drop, rhs=drop))
    # a row of a non-violated eigenvalue: the largest eigenpair of the first entry, inserted as one more row of it
    M, _ = multicut.lifted(S[0, :ks[0]], vv, n)
    w, V = np.linalg.eigh(M)
    assert w[-1] > 0
    co, rh = multicut.row_of(V[:, -1])
    at = int(e["n_offered"][0])
    c20 = np.zeros(20)
    c20[:co.shape[0]] = co
    with pytest.raises(AssertionError, match="not violated"):
        multicut.check_rows(*args, *broken(row_entry=lambda a: np.insert(a, at, 0), row_rank=lambda a: np.insert(a, at, at),
                                           row_lam=lambda a: np.insert(a, at, w[-1]), coef=lambda a: np.insert(a, at, c20, axis=0),
                                           rhs=lambda a: np.insert(a, at, rh)))
    # a row whose coefficients belong to another eigenvalue
    with pytest.raises(AssertionError):
        multicut.check_rows(*args, *broken(coef=swap, rhs=swap))


# ------------------------------------------------------------------------------------------ the layout
MULTI_COLS = ("idx", "score", "lam", "rhs", "row_lam", "values", "ks", "sets", "n_neg", "row_entry", "row_rank", "indptr", "indices", "bytes")
WRAPPER = r"""
#include "round_layout.h"
extern "C" void multi_batch(long m, const int64_t *in, int64_t *out)
{
    for (long i = 0; i < m; ++i) {
        const CsrMultiLayout y = csr_multi_layout(in[3 * i], in[3 * i + 1], (int)in[3 * i + 2]);
        const size_t v[%d] = { y.idx, y.score, y.lam, y.rhs, y.row_lam, y.values, y.ks, y.sets, y.n_neg, y.row_entry, y.row_rank, y.indptr,
                               y.indices, y.bytes };
        for (int j = 0; j < %d; ++j) out[%d * i + j] = (int64_t)v[j];
    }
}
""" % ((len(MULTI_COLS),) * 3)


def test_csr_multi_layout_arrays_are_aligned_disjoint_and_monotone(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text(WRAPPER)
    so = tmp_path / "layout.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    caps = (1, 2, 31, 32, 33, 64, 65, 129, 500, 5000, 16384)
    cases = []
    for c in caps:
        for rc in sorted(set([1, c - 1, c, c + 1, 2 * c, 5 * c - 1, 5 * c]) - {0}):
            for ld in (5, 9, 14, 20):
                cases.append((c, rc, ld))
    cases = np.ascontiguousarray(cases, dtype=np.int64)
    out = np.full((cases.shape[0], len(MULTI_COLS)), -99, dtype=np.int64)
    p64 = ctypes.POINTER(ctypes.c_int64)
    lib.multi_batch(ctypes.c_long(cases.shape[0]), cases.ctypes.data_as(p64), out.ctypes.data_as(p64))
    size_of = {}
    for (c, r, ld), row in zip(cases.tolist(), out.tolist()):
        y = dict(zip(MULTI_COLS, row))
        size = dict(idx=8 * c, score=8 * c, lam=8 * c, rhs=8 * r, row_lam=8 * r, values=8 * r * ld, ks=4 * c, sets=20 * c, n_neg=4 * c,
                    row_entry=4 * r, row_rank=4 * r, indptr=4 * (r + 1), indices=4 * r * ld)
        end = 128      # the header: completion word 7, rows 8, non-zeros 9, look-back mark 10, quota mark 11
        for name in MULTI_COLS[:-1]:
            assert y[name] % 8 == 0 and y[name] >= end, (name, c, r, ld)
            end = y[name] + size[name]
        assert y["bytes"] >= end and y["bytes"] % 8 == 0, (c, r, ld)
        size_of[(c, r, ld)] = y["bytes"]
    for (c, r, ld), b in size_of.items():      # monotone in cap and in row_cap
        for (c2, r2, ld2), b2 in size_of.items():
            if ld2 == ld and c2 >= c and r2 >= r:
                assert b2 >= b, ((c, r, ld), (c2, r2, ld2))


# ------------------------------------------------------------------------------------------ the C-ABI's new names
def test_new_names_in_header_binding_and_export_map():
    from sdpcutsel_via_nn_amd import _capi, multicut
    hdr = open(os.path.join(ROOT, "include", "sdpcut.h")).read()
    declared = set(re.findall(r"^(?:int|const char \*)\s*(sdpcut_\w+)\s*\(", hdr, flags=re.M))
    for name in ("sdpcut_round_csr_multi", "sdpcut_cut_rows_all"):
        assert name in declared and name in _capi.SIGNATURES
    exports = open(os.path.join(CSRC, "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", exports)
    assert pats and all(any(re.fullmatch(p.strip().replace("*", r"\w*"), name) for p in pats)
                        for name in ("sdpcut_round_csr_multi", "sdpcut_cut_rows_all"))
    assert int(re.search(r"#define SDPCUT_MULTI_MAX_PER_SET (\d+)", hdr).group(1)) == 5 == _capi.MULTI_MAX_PER_SET == multicut.MAX_PER_SET
    assert "sdpcut_round_multi_t" in hdr and "multirows.hip" in __import__("sdpcutsel_via_nn_amd.build", fromlist=["SOURCES"]).SOURCES
    # the binding's record: the plain round's record first, then the multi-cut fields
    f = dict(_capi.RoundMulti._fields_)
    assert _capi.RoundMulti._fields_[0] == ("csr", _capi.RoundCsr)
    assert [n for n, _ in _capi.RoundMulti._fields_[1:]] == ["row_cap", "n_used", "quota_hit", "reserved", "n_neg", "row_lam", "row_rank"]
    assert ctypes.sizeof(_capi.RoundMulti) == ctypes.sizeof(_capi.RoundCsr) + 8 + 8 + 4 + 4 + 3 * 8 and f["quota_hit"] is ctypes.c_int32
    assert _capi.SIGNATURES["sdpcut_round_csr_multi"][4:6] == [ctypes.c_int32, ctypes.c_int64]


# ------------------------------------------------------------------------------------------ argument checks without a device
def test_argument_checks_of_the_python_layer():
    from sdpcutsel_via_nn_amd import _capi, multicut
    import sdpcutsel_via_nn_amd as pkg
    assert _capi.check_multi_args(1, None, 64, 1) == (1, 64)
    assert _capi.check_multi_args(5, "sets", 64, 4) == (5, 320)
    assert _capi.check_multi_args(3, 7, 64, 2) == (3, 7)
    assert _capi.check_multi_args(2, 1) == (2, 1)
    for m in (0, 6, -1, 2.5):
        with pytest.raises(ValueError, match="cuts_per_set"):
            _capi.check_multi_args(m, None, 64, 1)
        with pytest.raises(ValueError, match="cuts_per_set"):
            multicut.expected(np.zeros((0, 5), np.int32), np.zeros(0, np.int32), np.zeros(3), 2, m)
    for q in (0, -3):
        with pytest.raises(ValueError, match="row_quota"):
            _capi.check_multi_args(2, q, 64, 1)
    with pytest.raises(ValueError, match="row_quota"):
        _capi.check_multi_args(2, "rows", 64, 1)
    with pytest.raises(ValueError, match="row_quota"):
        _capi.check_multi_args(2, None)
    for strat in (0, 5, -1, 104):
        with pytest.raises(ValueError, match="strategies"):
            _capi.check_multi_args(2, None, 64, strat)
    # the solver's front door: refused before anything touches a device or a file
    cs = pkg.CutSolver()
    assert cs.cuts_per_set == 1 and cs.cuts_row_quota is None
    with pytest.raises(AssertionError, match="max_parallel"):
        cs.cut_select_algo("no-such-file.in", 3, 0.1, strat=1, max_parallel=0.9, cuts_per_set=2)
    with pytest.raises(AssertionError, match="strategy 0"):
        cs.cut_select_algo("no-such-file.in", 3, 0.1, strat=0, cuts_per_set=2)
    with pytest.raises(ValueError, match="cuts_per_set"):
        cs.cut_select_algo("no-such-file.in", 3, 0.1, strat=1, cuts_per_set=6)
    with pytest.raises(AssertionError, match="row_quota"):
        cs.cut_select_algo("no-such-file.in", 3, 0.1, strat=1, cuts_per_set=2, row_quota=17)
    with pytest.raises(ValueError, match="cuts_per_set"):
        pkg.CutSolverQCQP().cut_select_algo("no-such-file.osil", 3, cuts_per_set=0)

    class _Ref(object):
        pass
    mod = type("m", (), {"CutSolver": _Ref})
    from sdpcutsel_via_nn_amd import cut_solver
    qp, _ = cut_solver.make_dropin_classes(mod, cuts_per_set=3)
    assert qp.cuts_per_set == 3 and cut_solver.make_dropin_classes(mod)[0].cuts_per_set == 1
    with pytest.raises(ValueError, match="cuts_per_set"):
        cut_solver.make_dropin_classes(mod, cuts_per_set=9)
