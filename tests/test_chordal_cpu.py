"""Chordal extension (sdpcut_chordal_extension) and the covers enumerated on it (sdpcut_enumerate_cover_ch: ch_ext 1, 2, -1 of
cut_select_qp.py:385-455) against numpy twins written here: the elimination game with the default greedy minimum-degree order,
and a per-edge restatement of the reference's dim-3 loops.  Host code only: no GPU."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN


# ----------------------------------------------------------------------------- twins
def _sym(A):
    A = np.asarray(A) != 0
    A = A | A.T
    A[np.diag_indices(A.shape[0])] = False
    return A


def twin_extension(A, order=None):
    """The elimination game: for each vertex v of the order its not-yet-eliminated neighbours in the current filled graph become
    a clique.  order None = at each step the not-yet-eliminated vertex with the fewest not-yet-eliminated neighbours, ties to the
    lowest index.  -> (filled graph, order used, number of fill edges)"""
    F = _sym(A).copy()
    n = F.shape[0]
    alive = np.ones(n, dtype=bool)
    used, fill = [], 0
    for step in range(n):
        if order is None:
            deg = (F & alive[None, :]).sum(axis=1)
            deg[~alive] = n + 1
            v = int(np.argmin(deg))          # first minimum = lowest index
        else:
            v = int(order[step])
        used.append(v)
        alive[v] = False
        nb = np.flatnonzero(F[v] & alive)
        missing = ~F[np.ix_(nb, nb)]
        missing[np.diag_indices(nb.size)] = False
        fill += int(missing.sum()) // 2
        F[np.ix_(nb, nb)] |= missing
    return F, np.array(used, dtype=np.int32), fill


def twin_cover3(E, O, ch_ext):
    """The dim-3 loops of cut_select_qp.py:405-449 edge by edge.  E = the pattern the cliques live in (the extended one for ch_ext
    1 and 2), O = the original pattern (read by ch_ext 2 only: a triangle counts with >= 2 of its 3 edges in O, a pair only if it
    is an edge of O).  -> (sets [N, 5] padded with -1, ks [N])"""
    n = E.shape[0]
    sets, ks = [], []
    for i1 in range(n):
        for i2 in np.flatnonzero(E[i1, i1 + 1:]) + i1 + 1:
            third = E[i1] & E[i2]
            if ch_ext == 2:
                third &= (O[i1, i2].astype(int) + O[i1].astype(int) + O[i2].astype(int)) >= 2
            third[[i1, i2]] = False
            fwd = np.flatnonzero(third[i2 + 1:]) + i2 + 1
            if fwd.size:
                rows = np.full((fwd.size, 5), -1, dtype=np.int32)
                rows[:, 0], rows[:, 1], rows[:, 2] = i1, i2, fwd
                sets.append(rows)
                ks.append(np.full(fwd.size, 3, dtype=np.int32))
            elif not third[:i2].any() and (ch_ext != 2 or O[i1, i2]):
                sets.append(np.array([[i1, i2, -1, -1, -1]], dtype=np.int32))
                ks.append(np.array([2], dtype=np.int32))
    if not sets:
        return np.zeros((0, 5), np.int32), np.zeros(0, np.int32)
    return np.concatenate(sets), np.concatenate(ks)


def _random_graph(n, dens, seed):
    rng = np.random.default_rng(seed)
    return _sym(np.triu(rng.uniform(size=(n, n)) < dens, 1))


def _graphs():
    out = []
    for n in (2, 7, 64, 65, 130, 300):
        for dens in (0.1, 0.5, 0.95):
            out.append(("n%d_d%g" % (n, dens), _random_graph(n, dens, 1000 * n + int(100 * dens))))
    for n in (7, 65):
        out.append(("n%d_empty" % n, np.zeros((n, n), dtype=bool)))
        out.append(("n%d_complete" % n, _sym(np.ones((n, n)))))
    return out


GRAPHS = _graphs()
_TRIPLES = {}


def _all_triples_twin(n):
    """the twin's P^E+_3 (the loops of ch_ext = 1 on the complete graph), computed once per n and left unchanged"""
    if n not in _TRIPLES:
        K = _sym(np.ones((n, n)))
        _TRIPLES[n] = twin_cover3(K, K, 1)
    return _TRIPLES[n]


def _enumerate_ch(ext, orig, ch_ext):
    """sdpcut_enumerate_cover_ch itself, through ctypes"""
    from sdpcutsel_via_nn_amd import _capi
    lib = _capi.load_library()
    u8p = ctypes.POINTER(ctypes.c_uint8)
    i32p = ctypes.POINTER(ctypes.c_int32)
    e = np.ascontiguousarray(ext, dtype=np.uint8) if ext is not None else None
    o = np.ascontiguousarray(orig, dtype=np.uint8) if orig is not None else None
    n = (e if e is not None else o).shape[0]
    ep = e.ctypes.data_as(u8p) if e is not None else None
    op = o.ctypes.data_as(u8p) if o is not None else None
    cnt = ctypes.c_int64(0)
    assert lib.sdpcut_enumerate_cover_ch(n, ep, op, ch_ext, 0, None, None, ctypes.byref(cnt)) == 0
    N = cnt.value
    S, ks = np.empty((max(N, 1), 5), dtype=np.int32), np.empty(max(N, 1), dtype=np.int32)
    assert lib.sdpcut_enumerate_cover_ch(n, ep, op, ch_ext, N, S.ctypes.data_as(i32p), ks.ctypes.data_as(i32p), ctypes.byref(cnt)) == 0
    assert cnt.value == N
    return S[:N], ks[:N]


def _is_peo(F, order):
    pos = np.empty(F.shape[0], dtype=int)
    pos[order] = np.arange(F.shape[0])
    for v in order:
        later = np.flatnonzero(F[v] & (pos > pos[v]))
        sub = F[np.ix_(later, later)]
        if int(sub.sum()) != later.size * (later.size - 1):
            return False
    return True


# ----------------------------------------------------------------------------- the extension
@pytest.mark.parametrize("name,A", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_extension_and_covers_equal_the_twins(name, A):
    """A chordal input gets zero fill WHEN ELIMINATED IN A PERFECT ELIMINATION ORDER (checked by feeding the extension back with
    the order that produced it); the greedy minimum-degree order is no such order in general -- a vertex of degree 2 joining two
    large cliques is picked first and fills one edge -- so with the default order zero fill is checked where it is certain: the
    empty and the complete graph."""
    import networkx as nx
    from sdpcutsel_via_nn_amd import _capi
    n = A.shape[0]
    ext, order, fill = _capi.chordal_extension(A)
    F, order_t, fill_t = twin_extension(A)
    assert ext.dtype == bool and np.array_equal(ext, F) and np.array_equal(order, order_t) and fill == fill_t
    assert np.array_equal(ext, ext.T) and not ext.diagonal().any()
    assert np.all(ext[A]) and fill == (int(ext.sum()) - int(A.sum())) // 2          # a superset: the original edges plus the fill
    assert sorted(order.tolist()) == list(range(n)) and _is_peo(ext, order)
    assert nx.is_chordal(nx.from_numpy_array(ext.astype(np.uint8)))
    if name.endswith(("empty", "complete")):
        assert fill == 0
    again, order2, fill2 = _capi.chordal_extension(ext, order=order)
    assert fill2 == 0 and np.array_equal(again, ext) and np.array_equal(order2, order)
    # a given order: the natural one and a random one
    for given in (np.arange(n), np.random.default_rng(n).permutation(n)):
        e2, o2, f2 = _capi.chordal_extension(A, order=given)
        F2, _, ft2 = twin_extension(A, given)
        assert np.array_equal(e2, F2) and np.array_equal(o2, given) and f2 == ft2
        assert _is_peo(e2, given)
    # the covers on it: same sets in the same order
    for ch_ext in (1, 2, -1):
        S, ks = _enumerate_ch(ext, A, ch_ext)
        S_t, ks_t = _all_triples_twin(n) if ch_ext == -1 else twin_cover3(ext, A, ch_ext)
        assert S.shape == S_t.shape and np.array_equal(S, S_t) and np.array_equal(ks, ks_t), (name, ch_ext)
        S2, ks2, N2 = _capi.enumerate_cover(A, 3, ch_ext=ch_ext)
        assert N2 == S_t.shape[0] and np.array_equal(S2, S_t) and np.array_equal(ks2, ks_t)
    S, ks = _enumerate_ch(None, A, 0)          # ch_ext = 0 is the cover of the original pattern
    S0, ks0, _ = _capi.enumerate_cover(A, 3)
    assert np.array_equal(S, S0) and np.array_equal(ks, ks0)
    S_t, ks_t = twin_cover3(A, A, 0)
    assert np.array_equal(S0, S_t) and np.array_equal(ks0, ks_t)


def test_ch_ext_1_at_dim_4_and_5_is_the_cover_of_the_extension():
    from sdpcutsel_via_nn_amd import _capi
    A = _random_graph(40, 0.15, 5)
    ext = _capi.chordal_extension(A)[0]
    for dim in (4, 5):
        S, ks, N = _capi.enumerate_cover(A, dim, ch_ext=1)
        S1, ks1, N1 = _capi.enumerate_cover(ext, dim)
        assert N == N1 and np.array_equal(S, S1) and np.array_equal(ks, ks1)
    assert _capi.enumerate_cover(A, 3, ch_ext=2, max_subs=1) == (None, None, _capi.enumerate_cover(A, 3, ch_ext=2)[2])


def test_refusals():
    from sdpcutsel_via_nn_amd import _capi
    A = _random_graph(12, 0.4, 1)
    for bad in ([0] * 12, list(range(11)) + [12], list(range(10)) + [3, 11], [-1] + list(range(1, 12))):
        with pytest.raises(ValueError):
            _capi.chordal_extension(A, order=bad)
    with pytest.raises(ValueError):
        _capi.chordal_extension(A, order=list(range(11)))
    with pytest.raises(ValueError):
        _capi.enumerate_cover(A, 4, ch_ext=2)          # the reference silently degrades this to ch_ext = 1
    with pytest.raises(ValueError):
        _capi.enumerate_cover(A, 4, ch_ext=-1)
    with pytest.raises(ValueError):
        _capi.enumerate_cover(A, 3, ch_ext=3)
    with pytest.raises(ValueError):
        _capi.chordal_extension(np.zeros((1025, 1025), dtype=bool))
    with pytest.raises(ValueError):
        _capi.chordal_extension(np.zeros((1, 1), dtype=bool))
    ext, order, fill = _capi.chordal_extension(np.zeros((1024, 1024), dtype=bool))
    assert fill == 0 and not ext.any() and np.array_equal(order, np.arange(1024))


# ----------------------------------------------------------------------------- pinned counts
def _instance(name):
    from sdpcutsel_via_nn_amd import harness
    return harness.parse_boxqp(os.path.join(GOLDEN, "instances", name))


@pytest.mark.parametrize("name,n1,n2,fill", [("spar020-100-1.in", 1105, 1105, 3), ("spar040-030-1.in", 3132, 1090, 247),
                                             ("spar070-050-1.in", 41019, 22705, 942)])
def test_pinned_counts_default_order(name, n1, n2, fill):
    """|P^bar(E)_3|, |bar(P*_3)| and the fill under the default order.  spar020-100-1: 1105 / 1105 are also the published
    nb_subproblems; spar040-030-1: published 3180 / 1075 (cvxopt's AMD is another order)."""
    from sdpcutsel_via_nn_amd import _capi
    adj = _instance(name)["adj"]
    assert _capi.chordal_extension(adj)[2] == fill
    assert _capi.enumerate_cover(adj, 3, ch_ext=1)[2] == n1
    assert _capi.enumerate_cover(adj, 3, ch_ext=2)[2] == n2


@pytest.mark.parametrize("name,n1,n2", [("spar020-100-1.in", 1140, 1139), ("spar040-030-1.in", 6890, 1477)])
def test_pinned_counts_natural_order(name, n1, n2):
    from sdpcutsel_via_nn_amd import _capi
    inst = _instance(name)
    nat = np.arange(inst["nb_vars"])
    assert _capi.enumerate_cover(inst["adj"], 3, ch_ext=1, order=nat)[2] == n1
    assert _capi.enumerate_cover(inst["adj"], 3, ch_ext=2, order=nat)[2] == n2


def test_all_triples():
    """P^E+_3 at n = 20: the 1140 triples in lexicographic order"""
    import itertools
    from sdpcutsel_via_nn_amd import _capi
    S, ks, N = _capi.enumerate_cover(np.zeros((20, 20)), 3, ch_ext=-1)
    assert N == 1140 and np.all(ks == 3) and np.all(S[:, 3:] == -1)
    assert [tuple(r) for r in S[:, :3].tolist()] == list(itertools.combinations(range(20), 3))


def test_cut_select_algo_refuses_other_flags():
    """the reference's assertion (cut_select_qp.py:94), raised before anything touches a device"""
    from sdpcutsel_via_nn_amd import cut_solver
    path = os.path.join(GOLDEN, "instances", "spar020-100-1.in")
    with pytest.raises(AssertionError, match="Chordal extension flags"):
        cut_solver.CutSolver().cut_select_algo(path, 3, 0.1, strat=1, nb_rounds_cuts=2, ch_ext=3)
