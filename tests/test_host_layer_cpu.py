"""CPU-side tests of the host layer above the C-ABI on the paths no device-free test reached: cut generation from a rank list
whose fused block is stale (the walk to (binding, ids) runs, ``Scorer.cut_rows`` / ``cut_rows_all``, the hand-over to both kinds
of row store), the triangle rows, and the round dicts ``Scorer`` builds from the library's records.  Fakes stand in for the
scorer and for the library; nothing here needs a GPU."""
import ctypes

import numpy as np
import pytest

from sdpcutsel_via_nn_amd import _capi, harness
from sdpcutsel_via_nn_amd.cut_solver import CutSolver, DeviceAgg, FeasEntry, _Binding

N_VARS, N_LIFTED = 12, 78
DROPPED = (1010, 1015, 23)           # ids whose smallest eigenvalue is not below -1e-15: no cut (cut_select_qp.py:743)


# ----------------------------------------------------------------------------- rows as functions of the candidate id
def _row(g):
    """(cols, coef, rhs) of candidate g's eigen-cut as the fake scorer hands it out: 2..5 variables, k(k+3)/2 entries"""
    k = 2 + g % 4
    w = k * (k + 3) // 2
    return [(7 * g + 3 * j) % 90 for j in range(w)], [g + j / 32.0 for j in range(w)], -g / 8.0


def _lam(g):
    return {DROPPED[0]: -1e-16, DROPPED[1]: 0.0, DROPPED[2]: 0.25}.get(g, -0.5 - g / 4096.0)


def _multi_count(g, m):
    return min(m, g % 3)


def _multi_row(g, r):
    cols, coef, rhs = _row(g)
    return cols, [v + 0.5 * r for v in coef], rhs - r


class _RowsScorer(object):
    """stands in for _capi.Scorer: a canned fused round, and cut rows derived from the ids it is asked about"""

    def __init__(self, name, base, scores, log):
        self.name, self.base, self.scores, self.log = name, base, np.asarray(scores, dtype=np.float64), log
        self.n = self.scores.shape[0]
        self.round_count, self.pending = 0, None

    def head_ids(self, w):
        return self.base + (np.arange(w, dtype=np.int64) * 5) % self.n

    def set_point(self, vv):
        pass

    def score(self, flags):
        raise AssertionError("nothing to score on these paths")

    def round_csr_begin(self, strat, sel, point=None):
        self.round_count += 1
        self.pending = object()
        self._args = (strat, sel)
        return self.pending

    def round_csr_end(self, copy=False):
        self.pending = None
        strat, sel = self._args
        w = min(sel, self.n)
        # the block's rows carry a sentinel: once the block is stale nothing of it may reach the LP
        return dict(idx=self.head_ids(w), score=self.scores[:w].copy(), lam=-np.ones(w), ks=np.full(w, 3, np.int32),
                    set_inds=np.array([[i % 7, i % 7 + 1, i % 7 + 2, -1, -1] for i in range(w)], dtype=np.int32).reshape(w, 5),
                    row_entry=np.arange(w, dtype=np.int32), indptr=np.arange(w + 1, dtype=np.int32) * 2,
                    indices=np.full(2 * w, 89, np.int32), values=np.full(2 * w, 777.0), rhs=np.full(w, 777.0), n_total=self.n,
                    new_strat=strat, counters=dict(nb_violated=w, strong=w, violated=w, nb_positive=w))

    def cut_rows(self, local_idx):
        idx = np.asarray(local_idx, dtype=np.int64)
        self.log.append((self.name, idx.tolist()))
        c = idx.shape[0]
        lam, coef, rhs = np.empty(c), np.full((c, 20), np.nan), np.empty(c)
        cols, ks = np.full((c, 20), -7, dtype=np.int64), np.empty(c, dtype=np.int32)
        for i, g in enumerate((idx + self.base).tolist()):
            cl, co, rh = _row(g)
            lam[i], rhs[i], ks[i] = _lam(g), rh, 2 + g % 4
            cols[i, :len(cl)], coef[i, :len(co)] = cl, co
        return lam, coef, rhs, cols, ks

    def cut_rows_all(self, local_idx, m):
        idx = np.asarray(local_idx, dtype=np.int64)
        self.log.append((self.name, idx.tolist(), m))
        c = idx.shape[0]
        gs = (idx + self.base).tolist()
        row_ptr = np.concatenate([[0], np.cumsum([_multi_count(g, m) for g in gs])]).astype(np.int64)
        n = int(row_ptr[-1])
        lam, coef, rhs = np.empty(n), np.full((n, 20), np.nan), np.empty(n)
        cols, ks = np.full((c, 20), -7, dtype=np.int64), np.empty(c, dtype=np.int32)
        for i, g in enumerate(gs):
            ks[i] = 2 + g % 4
            cols[i, :len(_row(g)[0])] = _row(g)[0]
            for r in range(_multi_count(g, m)):
                _, co, rh = _multi_row(g, r)
                p = int(row_ptr[i]) + r
                lam[p], rhs[p] = -1.0 - r, rh
                coef[p, :len(co)] = co
        return row_ptr, lam, coef, rhs, cols, ks


class _RefStore(object):
    """the reference's LP surface (cplex): add(lin_expr=, rhs=, senses=) only"""

    def __init__(self):
        self.calls = []

    def add(self, lin_expr=(), rhs=(), senses=()):
        self.calls.append((list(lin_expr), list(rhs), list(senses)))


class _Prob(object):
    def __init__(self):
        self.linear_constraints = _RefStore()


def _solver(kind, n_vars=N_VARS):
    cs = CutSolver()
    cs._gpu_overlap = False
    cs._nb_vars, cs._nb_lifted, cs._dim = n_vars, n_vars * (n_vars + 1) // 2, 3
    cs._sparse_pair = harness.SparsePair
    cs._gpu_bindings = {}
    cs._my_prob = harness.LinearRelaxation(np.zeros(cs._nb_lifted + n_vars)) if kind == "csr" else _Prob()
    return cs


def _bind(cs, sc):
    agg = DeviceAgg(sc, sc.n, N_VARS)
    b = _Binding(sc, agg, N_VARS, N_LIFTED)
    b.n_at_bind, b.serial = sc.n, 0
    cs._gpu_bindings[id(agg)] = b
    return agg, b


def _stale_rank_list(cs, agg, strat, vv):
    """the list's ranking through the fused round, whose block the scorer has since overwritten"""
    cs._agg_list = agg
    rl = cs._sel_eigcut_by_ordering_on_measure(strat, vv, 1)
    assert rl._fused is not None and rl.fused_rows(1) is not None
    rl._b.scorer.round_count += 1
    assert rl.fused_rows(1) is None
    return rl


def _stored(cs):
    """what the LP received: ([(ind, val) per row], rhs, senses, number of add calls on a reference-style store)"""
    store = cs._my_prob.linear_constraints
    if isinstance(store, _RefStore):
        rows = [(r.ind, r.val) for c in store.calls for r in c[0]]
        return rows, [v for c in store.calls for v in c[1]], [v for c in store.calls for v in c[2]], len(store.calls)
    return [(r.ind, r.val) for r in store.rows], store.rhs, store.senses, None


def _expected(ids):
    keep = [g for g in ids if g not in DROPPED]
    return [(_row(g)[0], _row(g)[1]) for g in keep], [_row(g)[2] for g in keep], ["G"] * len(keep)


def _check_store(cs, ids, returned):
    rows, rhs, senses, calls = _stored(cs)
    exp = _expected(ids)
    assert (rows, rhs, senses) == exp and returned == len(exp[0])
    if calls is not None:
        assert calls >= 1
        assert all(type(i) is int for ind, _ in rows for i in ind) and all(type(v) is float for _, val in rows for v in val)
        assert all(type(v) is float for v in rhs)


SCORES_A = [9.0, 8.0, 7.0, 6.0, 0.0, 5.0, -1.0, 4.0, 3.0, 2.0, 1.0, 0.5, 0.25, 0.125, 0.1, 0.05]
STORES = ("csr", "ref")


def _setup(kind):
    cs, log = _solver(kind), []
    sa, sb = _RowsScorer("A", 1000, SCORES_A, log), _RowsScorer("B", 1000, np.linspace(3.0, 1.0, 21), log)
    (agg_a, ba), (agg_b, bb) = _bind(cs, sa), _bind(cs, sb)
    rng = np.random.default_rng(3)
    return cs, log, (sa, agg_a, ba), (sb, agg_b, bb), rng.random(90), rng.random(90)


@pytest.mark.parametrize("kind", STORES)
def test_stale_rank_list_goes_through_the_walk_and_cut_rows(kind):
    cs, log, (sa, agg_a, ba), _, vv, vv2 = _setup(kind)
    rl = _stale_rank_list(cs, agg_a, 2, vv)
    ids = sa.head_ids(16).tolist()
    assert 1010 in ids[:6] and 1015 in ids[:6]
    nb = cs._gen_eigcuts_selected(2, 6, rl, vars_values=vv2)
    assert log == [("A", [g - 1000 for g in ids[:6]])]
    _check_store(cs, ids[:6], nb)
    assert nb == 4
    # optimality cuts are generated at the point the list was ranked at, whatever the caller passes (cut_select_qp.py:735-741)
    assert np.array_equal(ba.point_copy, vv)


@pytest.mark.parametrize("kind", STORES)
def test_strong_only_head_stops_before_the_first_nonpositive_score(kind):
    cs, log, (sa, agg_a, ba), _, vv, _ = _setup(kind)
    rl = _stale_rank_list(cs, agg_a, 2, vv)
    ids = sa.head_ids(16).tolist()
    nb = cs._gen_eigcuts_selected(2, 9, rl[0:9], strong_only=True, vars_values=vv)
    assert log == [("A", [g - 1000 for g in ids[:4]])]           # SCORES_A[4] == 0
    _check_store(cs, ids[:4], nb)
    # a feasibility list is not cut short (:725 tests the strategy)
    cs2, log2, _, (sb, agg_b, bb), vv, _ = _setup(kind)
    rl1 = _stale_rank_list(cs2, agg_b, 1, vv)
    nb = cs2._gen_eigcuts_selected(1, 5, rl1[0:5], strong_only=True, vars_values=vv)
    assert log2 == [("B", [g - 1000 for g in sb.head_ids(5).tolist()])]
    _check_store(cs2, sb.head_ids(5).tolist(), nb)


@pytest.mark.parametrize("kind", STORES)
def test_plain_list_of_optimality_tuples(kind):
    cs, log, (sa, agg_a, ba), _, vv, _ = _setup(kind)
    cs._agg_list = agg_a
    ids = [1003, 1010, 1001, 1015, 1002, 1007]
    entries = [(g, s, (), ()) for g, s in zip(ids, [5.0, 4.0, 3.0, 2.0, -1.0, 1.0])]
    nb = cs._gen_eigcuts_selected(2, 5, entries, vars_values=vv)
    assert log == [("A", [g - 1000 for g in ids[:5]])]
    _check_store(cs, ids[:5], nb)
    assert np.array_equal(ba.point_copy, vv)
    cs, log, (sa, agg_a, ba), _, vv, _ = _setup(kind)
    cs._agg_list = agg_a
    nb = cs._gen_eigcuts_selected(4, 6, entries, strong_only=True, vars_values=vv)
    assert log == [("A", [g - 1000 for g in ids[:4]])]
    _check_store(cs, ids[:4], nb)


def _feas(ids_bindings):
    return [FeasEntry(([0, 1, 2], 1.0, [0, 1, 2, 12, 13, 23], 3), g, b) for g, b in ids_bindings]


@pytest.mark.parametrize("kind", STORES)
def test_feasibility_entries_of_two_bindings_run_by_run(kind):
    cs, log, (sa, agg_a, ba), (sb, agg_b, bb), vv, _ = _setup(kind)
    cs._agg_list = agg_a
    entries = _feas([(1004, ba), (1010, ba), (1019, bb), (1002, ba), (1001, bb)])
    nb = cs._gen_eigcuts_selected(1, 4, entries, vars_values=vv)
    assert log == [("A", [4, 10]), ("B", [19]), ("A", [2])]
    _check_store(cs, [1004, 1010, 1019, 1002], nb)
    assert np.array_equal(ba.point_copy, vv) and np.array_equal(bb.point_copy, vv)


@pytest.mark.parametrize("kind", STORES)
def test_head_of_a_concatenation_of_two_stale_rank_lists(kind):
    """(A + B)[0:s] of cut_select_qcqp.py:79 under strategy 1: the cuts of each part, in list order, at the caller's point"""
    cs, log, (sa, agg_a, ba), (sb, agg_b, bb), vv, vv2 = _setup(kind)
    ra, rb = _stale_rank_list(cs, agg_a, 1, vv), _stale_rank_list(cs, agg_b, 1, vv)
    ids = sa.head_ids(16).tolist() + sb.head_ids(9).tolist()
    nb = cs._gen_eigcuts_selected(1, 25, (ra + rb)[0:25], vars_values=vv2)
    assert log == [("A", [g - 1000 for g in ids[:16]]), ("B", [g - 1000 for g in ids[16:]])]
    _check_store(cs, ids, nb)
    assert np.array_equal(ba.point_copy, vv2) and np.array_equal(bb.point_copy, vv2)


@pytest.mark.parametrize("kind", STORES)
def test_random_strategy_takes_the_shuffled_list_itself(kind):
    cs, log = _solver(kind), []
    sc = _RowsScorer("R", 0, np.zeros(40), log)
    agg = [([0, 1, 2], [0, 1, 2, 12, 13, 23])] * 40
    b = _Binding(sc, agg, N_VARS, N_LIFTED)
    b.n_at_bind, b.serial = 40, 0
    cs._gpu_bindings[id(agg)] = b
    cs._agg_list = agg
    nb = cs._gen_eigcuts_selected(5, 26, agg, vars_values=np.linspace(0, 1, 90))
    assert log == [("R", list(range(26)))]
    _check_store(cs, list(range(26)), nb)
    assert nb == 25                                               # id 23 has a positive smallest eigenvalue


@pytest.mark.parametrize("kind", STORES)
def test_empty_selection_hands_over_nothing_once(kind):
    cs, log, (sa, agg_a, ba), _, vv, _ = _setup(kind)
    rl = _stale_rank_list(cs, agg_a, 2, vv)
    assert cs._gen_eigcuts_selected(2, 0, rl, vars_values=vv) == 0 and log == []
    rows, rhs, senses, calls = _stored(cs)
    assert rows == [] and rhs == [] and senses == [] and calls in (None, 1)
    if kind == "ref":
        assert cs._my_prob.linear_constraints.calls == [([], [], [])]
    else:
        assert cs._my_prob.linear_constraints.get_num() == 0


# ----------------------------------------------------------------------------- the same lists with cuts_per_set = 2
def _multi_expected(ids, m, quota):
    rows, per_entry = [], []
    for g in ids:
        per_entry.append(_multi_count(g, m))
        rows.extend(_multi_row(g, r) for r in range(per_entry[-1]))
    offered = len(rows)
    kept = rows[:quota]
    starts = np.concatenate([[0], np.cumsum(per_entry)[:-1]]) if ids else np.zeros(0)
    used = sum(1 for n, s in zip(per_entry, starts) if n > 0 and s < len(kept))
    hist = np.bincount(np.array(per_entry, dtype=np.int64), minlength=m + 1).tolist()
    rec = dict(entries=len(ids), entries_used=used, rows=len(kept), offered=offered, offered_hist=hist, quota=quota, quota_hit=offered > quota)
    return [(c, v) for c, v, _ in kept], [r for _, _, r in kept], ["G"] * len(kept), rec


def _check_multi(cs, strat, ids, quota, returned):
    rows, rhs, senses, calls = _stored(cs)
    e_rows, e_rhs, e_senses, rec = _multi_expected(ids, 2, quota)
    assert (rows, rhs, senses) == (e_rows, e_rhs, e_senses) and returned == len(e_rows)
    assert cs.multi_log[-1] == dict(rec, strat=strat)
    if calls is not None:
        assert calls == 1
        assert all(type(i) is int for ind, _ in rows for i in ind) and all(type(v) is float for _, val in rows for v in val)
        assert all(type(v) is float for v in rhs)


@pytest.mark.parametrize("kind", STORES)
@pytest.mark.parametrize("row_quota", (None, "sets"))
def test_multi_cut_rows_of_a_stale_rank_list_keep_the_quota_in_list_order(kind, row_quota):
    cs, log, (sa, agg_a, ba), _, vv, vv2 = _setup(kind)
    cs.cuts_per_set, cs.cuts_row_quota, cs.multi_log = 2, row_quota, []
    rl = _stale_rank_list(cs, agg_a, 2, vv)
    ids = sa.head_ids(16).tolist()
    nb = cs._gen_eigcuts_selected(2, 6, rl, vars_values=vv2)
    assert log == [("A", [g - 1000 for g in ids[:6]], 2)]
    _check_multi(cs, 2, ids[:6], 12 if row_quota == "sets" else 6, nb)
    assert cs.multi_log[-1]["quota_hit"] == (row_quota is None) and len(cs.multi_log) == 1
    assert np.array_equal(ba.point_copy, vv2)                     # the multi path prefers the caller's point


@pytest.mark.parametrize("kind", STORES)
def test_multi_cut_rows_of_entry_runs_concatenations_and_the_shuffled_list(kind):
    cs, log, (sa, agg_a, ba), (sb, agg_b, bb), vv, _ = _setup(kind)
    cs.cuts_per_set, cs.multi_log = 2, []
    cs._agg_list = agg_a
    entries = _feas([(1004, ba), (1010, ba), (1019, bb), (1002, ba), (1001, bb)])
    nb = cs._gen_eigcuts_selected(1, 4, entries, vars_values=vv)
    assert log == [("A", [4, 10], 2), ("B", [19], 2), ("A", [2], 2)]
    _check_multi(cs, 1, [1004, 1010, 1019, 1002], 4, nb)

    cs, log, (sa, agg_a, ba), (sb, agg_b, bb), vv, _ = _setup(kind)
    cs.cuts_per_set, cs.cuts_row_quota, cs.multi_log = 2, "sets", []
    ra, rb = _stale_rank_list(cs, agg_a, 1, vv), _stale_rank_list(cs, agg_b, 1, vv)
    ids = sa.head_ids(16).tolist() + sb.head_ids(9).tolist()
    nb = cs._gen_eigcuts_selected(1, 25, (ra + rb)[0:25], vars_values=vv)
    assert log == [("A", [g - 1000 for g in ids[:16]], 2), ("B", [g - 1000 for g in ids[16:]], 2)]
    _check_multi(cs, 1, ids, 50, nb)

    cs, log = _solver(kind), []
    cs.cuts_per_set, cs.multi_log = 2, []
    sc = _RowsScorer("R", 0, np.zeros(40), log)
    agg = [([0, 1, 2], [0, 1, 2, 12, 13, 23])] * 40
    b = _Binding(sc, agg, N_VARS, N_LIFTED)
    b.n_at_bind, b.serial = 40, 0
    cs._gpu_bindings[id(agg)] = b
    cs._agg_list = agg
    nb = cs._gen_eigcuts_selected(5, 9, agg, vars_values=np.linspace(0, 1, 90))
    assert log == [("R", list(range(9)), 2)]
    _check_multi(cs, 5, list(range(9)), 9, nb)


@pytest.mark.parametrize("kind", STORES)
def test_multi_cut_rows_of_nothing(kind):
    """strong_only on a list whose first score is not positive: no entry, one empty hand-over, a record of zeros"""
    cs, log = _solver(kind), []
    cs.cuts_per_set, cs.multi_log = 2, []
    sc = _RowsScorer("Z", 1000, [0.0, -1.0, -2.0], log)
    agg, b = _bind(cs, sc)
    rl = _stale_rank_list(cs, agg, 2, np.linspace(0, 1, 90))
    assert cs._gen_eigcuts_selected(2, 3, rl[0:3], strong_only=True, vars_values=np.linspace(0, 1, 90)) == 0
    assert log == []
    assert cs.multi_log == [dict(strat=2, entries=0, entries_used=0, rows=0, offered=0, offered_hist=[0, 0, 0], quota=3, quota_hit=False)]
    rows, rhs, senses, calls = _stored(cs)
    assert rows == [] and rhs == [] and senses == []
    if kind == "ref":
        assert cs._my_prob.linear_constraints.calls == [([], [], [])]


# ----------------------------------------------------------------------------- triangle rows
class _FakeTri(object):
    def __init__(self, ent, nb_viol):
        self.ent, self.nb_viol, self.points, self.asked = np.asarray(ent, dtype=np.int64), nb_viol, [], []

    def set_point(self, vv):
        self.points.append(np.array(vv))

    def tri_separate(self, max_out):
        self.asked.append(max_out)
        return self.ent.copy(), np.linspace(1.0, 0.5, self.ent.shape[0]), self.nb_viol


TRIPLES = np.array([[0, 1, 2], [0, 2, 5], [1, 3, 4], [2, 4, 5], [0, 3, 5]], dtype=np.int32)
TRI_ENT = [4 * 1 + 3, 4 * 0 + 0, 4 * 2 + 1, 4 * 4 + 2, 4 * 3 + 3, 4 * 2 + 0, 4 * 1 + 1]


def _tri_rows_one_by_one(entries, n):
    """the rows as cut_select_qp.py:846-861 builds them"""
    L = n * (n + 1) // 2
    coeffs = {0: [-1, -1, 1, 1], 1: [-1, 1, -1, 1], 2: [1, -1, -1, 1], 3: [1, 1, 1, -1, -1, -1]}
    rows, rhs = [], []
    for e in entries:
        set_inds, t = TRIPLES[e >> 2].tolist(), e & 3
        Xarr = [n * set_inds[a] - set_inds[a] * (set_inds[a] + 1) // 2 + set_inds[b] for a in range(3) for b in range(a, 3)]
        if t == 3:
            rows.append(([Xarr[1], Xarr[2], Xarr[4], set_inds[0] + L, set_inds[1] + L, set_inds[2] + L], coeffs[3]))
            rhs.append(-1)
        else:
            rows.append(([Xarr[1], Xarr[2], Xarr[4], set_inds[t] + L], coeffs[t]))
            rhs.append(0)
    return rows, rhs


@pytest.mark.parametrize("kind", STORES)
@pytest.mark.parametrize("sel_size, nb_viol, expect", ((0.5, 7, 7), (3, 2, 6), (0.5, 0, 0)))
def test_triangle_rows(kind, sel_size, nb_viol, expect):
    """nb_tri_cuts of cut_select_qp.py:843-844: min(MAX, violated) decides at a fraction, min(MIN, floor(sel_size * violated)) at
    a number of cuts; every inequality type, on both kinds of row store"""
    n = 6
    cs = _solver(kind, n_vars=n)
    cs._gpu_tri, cs._gpu_tri_triples, cs._gpu_tri_triples64 = _FakeTri(TRI_ENT, nb_viol), TRIPLES, None
    vv = np.linspace(0, 1, 27)
    nb = cs._separate_and_add_triangle(sel_size, vv)
    assert nb == expect and cs._gpu_tri.asked == [cs._TRI_CUTS_PER_ROUND_MAX] and np.array_equal(cs._gpu_tri.points[0], vv)
    rows, rhs, senses, calls = _stored(cs)
    e_rows, e_rhs = _tri_rows_one_by_one(TRI_ENT[:expect], n)
    assert rows == e_rows and rhs == e_rhs and senses == ["G"] * expect
    if expect:
        assert {len(r[0]) for r in rows} == {4, 6} and {e & 3 for e in TRI_ENT[:expect]} == {0, 1, 2, 3}
    if calls is not None:
        assert calls == 1
        # the reference hands integer coefficients and right-hand sides (:846, :855, :860)
        assert all(type(i) is int for ind, _ in rows for i in ind) and all(type(v) is int for _, val in rows for v in val)
        assert all(type(v) is int for v in rhs)
        if not expect:
            assert cs._my_prob.linear_constraints.calls == [([], [], [])]


# ----------------------------------------------------------------------------- Scorer round dicts from a fake library
CAP, LD, N_OUT, N_ROWS = 8, 20, 5, 4
ROUND_KEYS = {"idx": np.int64, "score": np.float64, "lam": np.float64, "ks": np.int32, "set_inds": np.int32, "row_entry": np.int32,
              "indptr": np.int32, "indices": np.int32, "values": np.float64, "rhs": np.float64}
COUNTERS = dict(nb_violated=11, strong=12, violated=13, nb_positive=14)


def _round_arrays(row_cap=CAP, seed=0):
    """backing arrays of one round at their capacities, as the library lays them out in its pinned block"""
    rng = np.random.default_rng(seed)
    a = dict(idx=rng.integers(0, 1000, CAP), score=rng.random(CAP), lam=-rng.random(CAP), ks=rng.integers(2, 6, CAP).astype(np.int32),
             set_inds=rng.integers(0, 12, (CAP, 5)).astype(np.int32), row_entry=np.zeros(row_cap, np.int32),
             indptr=np.zeros(row_cap + 1, np.int32), indices=rng.integers(0, 90, row_cap * LD).astype(np.int32),
             values=rng.random(row_cap * LD), rhs=-rng.random(row_cap))
    a["row_entry"][:N_ROWS] = [0, 1, 3, 4]
    a["indptr"][:N_ROWS + 1] = [0, 2, 5, 7, 10]
    return a


def _fill_csr(o, a, empty=False):
    o.cap, o.n_out, o.n_total, o.new_strat, o.row_ld = (0 if empty else CAP), (0 if empty else N_OUT), 321, 1, LD
    for i, v in enumerate((11, 12, 13, 14)):
        o.counters[i] = v
    o.n_rows, o.nnz = (0, 0) if empty else (N_ROWS, 10)
    for f, k in (("idx", "idx"), ("score", "score"), ("lam_min", "lam"), ("ks", "ks"), ("set_inds", "set_inds"), ("row_entry", "row_entry"),
                 ("indptr", "indptr"), ("indices", "indices"), ("values", "values"), ("rhs", "rhs")):
        setattr(o, f, a[k].ctypes.data)


def _round_expected(a, empty=False):
    w, r, nnz = (0, 0, 0) if empty else (N_OUT, N_ROWS, 10)
    e = {k: a[k][:w] for k in ("idx", "score", "lam", "ks", "set_inds")}
    e.update(row_entry=a["row_entry"][:r], indptr=a["indptr"][:r + 1] if not empty else np.zeros(1, np.int32),
             indices=a["indices"][:nnz], values=a["values"][:nnz], rhs=a["rhs"][:r])
    return e


class _FakeLib(object):
    """stands in for libsdpcut_hip.so: fills the out-records from numpy arrays it keeps alive"""

    def __init__(self):
        self.a = _round_arrays()
        self.multi = dict(_round_arrays(row_cap=2 * CAP, seed=1), n_neg=np.array([1, 1, 0, 1, 1, 0, 0, 0], np.int32),
                          row_lam=-np.arange(1.0, 2 * CAP + 1), row_rank=np.zeros(2 * CAP, np.int32))
        self.empty, self.calls = False, []
        self.dense = dict(eigvals=np.linspace(-1, 1, 13), cols=np.arange(90, dtype=np.int32)[::-1].copy(), values=np.arange(270.0).reshape(3, 90),
                          rhs=-np.arange(3.0))
        self.pool = dict(leave=np.array([5, 9], np.int64), enter=np.array([2, 7, 3], np.int64), dropped=np.array([1], np.int64),
                         enter_indptr=np.array([0, 2, 4, 7], np.int32), enter_indices=np.arange(7, dtype=np.int32),
                         enter_values=np.arange(7.0) / 4, enter_rhs=-np.arange(3.0), enter_sense=np.array([1, -1, 1], np.int32),
                         enter_key=np.array([3.0, 2.0, 1.0]))
        # the batch block of round_csr_points: ONE buffer, record 0 a full round and record 1 an empty one
        sizes = [("idx", 8 * CAP), ("score", 8 * CAP), ("lam", 8 * CAP), ("ks", 4 * CAP), ("set_inds", 20 * CAP), ("row_entry", 4 * CAP),
                 ("indptr", 4 * CAP + 8), ("values", 8 * CAP * LD), ("rhs", 8 * CAP), ("indices", 4 * CAP * LD)]
        self.block = np.zeros(sum(s for _, s in sizes) // 8 + 1, dtype=np.int64)
        self.batch, off = {}, 0
        for k, s in sizes:
            shape = (CAP, 5) if k == "set_inds" else -1
            self.batch[k] = self.block.view(np.uint8)[off:off + s].view(ROUND_KEYS[k]).reshape(shape)
            self.batch[k].reshape(-1)[:self.a[k].size] = self.a[k].reshape(-1)
            off += s

    def sdpcut_last_error(self, h):
        return b"fake"

    def sdpcut_round_csr(self, h, vv, strat, sel, out):
        self.calls.append(("round_csr", strat, sel, bool(vv)))
        _fill_csr(out._obj, self.a, self.empty)
        return 0

    def sdpcut_round_csr_diverse(self, h, vv, strat, sel, pool, mp, out, info):
        self.calls.append(("diverse", strat, sel, pool, mp))
        _fill_csr(out._obj, self.a, self.empty)
        i = info._obj
        i.pool, i.examined, i.skipped_nonviolated, i.rejected_parallel = pool, 7, 1, 2
        return 0

    def sdpcut_round_csr_multi(self, h, vv, strat, sel, m, quota, out):
        self.calls.append(("multi", strat, sel, m, quota))
        o = out._obj
        _fill_csr(o.csr, self.multi, self.empty)
        o.row_cap, o.n_used, o.quota_hit = quota, 0 if self.empty else 4, 0 if self.empty else 1
        o.n_neg, o.row_lam, o.row_rank = (self.multi[k].ctypes.data for k in ("n_neg", "row_lam", "row_rank"))
        return 0

    def sdpcut_round_csr_points(self, h, P, pts, ld, strat, sel, recs):
        self.calls.append(("points", P, ld, strat, sel))
        for p in range(P):
            _fill_csr(recs[p], self.batch, empty=(p == 1))
        return 0

    def sdpcut_dense_round(self, h, vv, out):
        o, d = out._obj, self.dense
        o.dim, o.n_rows, o.sweeps, o.row_len = 13, 0 if self.empty else 3, 6, 90
        o.eigvals, o.cols, o.values, o.rhs = (d[k].ctypes.data for k in ("eigvals", "cols", "values", "rhs"))
        return 0

    def sdpcut_pool_step(self, h, vv, par, out):
        p, o, d = par._obj, out._obj, self.pool
        self.calls.append(("pool_step", p.tight_tol, p.viol_tol, p.max_age, p.drop_age, p.max_return))
        e = self.empty
        o.n_in_lp, o.n_parked, o.n_violated, o.n_dropped = 40, 6, 0 if e else 5, 0 if e else 1
        o.n_leave, o.n_enter, o.enter_nnz = (0, 0, 0) if e else (2, 3, 7)
        for k, arr in d.items():
            setattr(o, k, arr.ctypes.data)
        return 0


def _scorer():
    sc = _capi.Scorer.__new__(_capi.Scorer)
    sc._lib, sc._h, sc.nb_vars, sc.round_count = _FakeLib(), ctypes.c_void_p(1), N_VARS, 0
    sc.pool_capacity, sc._pool_rows = 64, 50
    return sc


POINT = np.linspace(0, 1, N_LIFTED + N_VARS)
ROUND_CALLS = {
    "round_csr": lambda sc, point=POINT, **k: sc.round_csr(2, 5, point=point, **k),
    "round_csr_diverse": lambda sc, point=POINT, **k: sc.round_csr_diverse(point, 2, 5, 0.9, **k),
    "round_csr_multi": lambda sc, point=POINT, **k: sc.round_csr_multi(point, 2, 5, 2, row_quota="sets", **k),
}


def _check_arrays(res, expected, dtypes):
    for k, e in expected.items():
        assert res[k].dtype == dtypes[k] and res[k].shape == e.shape and np.array_equal(res[k], e), k


def _multi_expected_dict(a, empty=False):
    w, r = (0, 0) if empty else (N_OUT, N_ROWS)
    return dict(_round_expected(a, empty), n_neg=a["n_neg"][:w], row_lam=a["row_lam"][:r], row_rank=a["row_rank"][:r])


MULTI_KEYS = dict(ROUND_KEYS, n_neg=np.int32, row_lam=np.float64, row_rank=np.int32)


@pytest.mark.parametrize("name", sorted(ROUND_CALLS))
def test_scorer_round_dicts(name):
    sc, call = _scorer(), ROUND_CALLS[name]
    lib = sc._lib
    multi = name == "round_csr_multi"
    backing, dtypes = (lib.multi, MULTI_KEYS) if multi else (lib.a, ROUND_KEYS)
    expected = (lambda empty=False: _multi_expected_dict(backing, empty)) if multi else (lambda empty=False: _round_expected(backing, empty))
    scalars = dict(n_total=321, new_strat=1, counters=COUNTERS)
    if multi:
        scalars.update(n_used=4, quota_hit=True, row_cap=10)
    if name == "round_csr_diverse":
        scalars.update(info=dict(pool=20, examined=7, skipped_nonviolated=1, rejected_parallel=2))
    res = call(sc)
    assert set(res) == set(dtypes) | set(scalars) and sc.round_count == 1
    _check_arrays(res, expected(), dtypes)
    for k, v in scalars.items():
        assert res[k] == v and type(res[k]) is type(v), k
    assert all(type(v) is int for v in res["counters"].values())
    # views of the library's block: a second round on the same block returns equal views of the same memory
    again = call(sc)
    assert sc.round_count == 2
    for k in dtypes:
        assert np.array_equal(again[k], res[k]) and again[k].ctypes.data == res[k].ctypes.data, k
    detached = call(sc, copy=True)
    keep = {k: detached[k].copy() for k in dtypes}
    backing["score"][:] += 1.0
    backing["values"][:] += 1.0
    backing["rhs"][:] -= 1.0
    assert np.array_equal(res["score"], backing["score"][:N_OUT]) and np.array_equal(res["values"], backing["values"][:10])
    _check_arrays(detached, keep, dtypes)
    assert not np.array_equal(detached["values"], res["values"])
    # point=None keeps the device's point: a null pointer goes down
    call(sc, point=None)
    assert lib.calls[-1][0] in ("round_csr", "diverse", "multi")
    # the empty round
    lib.empty = True
    res = call(sc)
    _check_arrays(res, expected(True), dtypes)
    assert res["indptr"].tolist() == [0] and res["set_inds"].shape == (0, 5) and res["n_total"] == 321 and res["counters"] == COUNTERS
    if multi:
        assert res["n_used"] == 0 and res["quota_hit"] is False
    with pytest.raises(ValueError):
        call(sc, point=POINT[:-1])
    if name != "round_csr":
        sc._h = None
        with pytest.raises(_capi.SdpCutError, match="closed"):
            call(sc)


def test_plain_and_multi_rounds_share_a_block_but_not_its_layout():
    """the library writes both kinds of round into the same pinned block: same address of ``idx``, same capacities, other
    offsets for the arrays behind it; a multi-cut round right after a plain one must not read the plain round's arrays"""
    sc = _scorer()
    lib = sc._lib
    for k in ("idx", "score", "lam"):
        lib.multi[k] = lib.a[k]
    plain = sc.round_csr(2, CAP, point=POINT)
    res = sc.round_csr_multi(POINT, 2, CAP, 2)                     # row_quota None: the row capacity is the head's
    assert res["row_cap"] == CAP and res["idx"].ctypes.data == plain["idx"].ctypes.data
    _check_arrays(res, _multi_expected_dict(lib.multi), MULTI_KEYS)
    _check_arrays(sc.round_csr(2, CAP, point=POINT), _round_expected(lib.a), ROUND_KEYS)


def test_scorer_round_dicts_of_a_batch():
    sc = _scorer()
    lib = sc._lib
    pts = np.stack([POINT, POINT[::-1]])
    res = sc.round_csr_points(pts, 2, 5)
    assert len(res) == 2 and sc.round_count == 1 and lib.calls[-1] == ("points", 2, 90, 2, 5)
    for d, empty in zip(res, (False, True)):
        assert set(d) == set(ROUND_KEYS) | {"n_total", "new_strat", "counters"}
        _check_arrays(d, _round_expected(lib.batch, empty), ROUND_KEYS)
        assert d["n_total"] == 321 and d["new_strat"] == 1 and d["counters"] == COUNTERS
        assert all(type(v) is int for v in d["counters"].values()) and type(d["n_total"]) is int
    assert res[1]["indptr"].tolist() == [0] and res[1]["set_inds"].shape == (0, 5)
    again = sc.round_csr_points(pts, 2, 5)
    for k in ROUND_KEYS:
        assert np.array_equal(again[0][k], res[0][k]) and again[0][k].ctypes.data == res[0][k].ctypes.data
    detached = sc.round_csr_points(pts, 2, 5, copy=True)
    keep = detached[0]["values"].copy()
    lib.batch["values"][:] += 1.0
    assert np.array_equal(res[0]["values"], lib.batch["values"][:10]) and np.array_equal(detached[0]["values"], keep)
    with pytest.raises(ValueError):
        sc.round_csr_points(pts[:, :-1], 2, 5)
    with pytest.raises(ValueError):
        sc.round_csr_points(POINT, 2, 5)
    sc._h = None
    with pytest.raises(_capi.SdpCutError, match="closed"):
        sc.round_csr_points(pts, 2, 5)


def test_scorer_dense_round_dict():
    sc = _scorer()
    d = sc._lib.dense
    res = sc.dense_round(POINT)
    assert set(res) == {"eigvals", "cols", "values", "rhs", "n_rows", "sweeps"} and sc.round_count == 1
    _check_arrays(res, d, dict(eigvals=np.float64, cols=np.int32, values=np.float64, rhs=np.float64))
    assert res["n_rows"] == 3 and res["sweeps"] == 6 and type(res["n_rows"]) is int
    again = sc.dense_round(POINT)
    assert all(np.array_equal(again[k], res[k]) and again[k].ctypes.data == res[k].ctypes.data for k in d)
    detached = sc.dense_round(POINT, copy=True)
    d["values"][:] += 1.0
    assert np.array_equal(res["values"], d["values"]) and np.array_equal(detached["values"], d["values"] - 1.0)
    sc._lib.empty = True
    res = sc.dense_round()
    assert res["n_rows"] == 0 and res["values"].shape == (0, 90) and res["rhs"].shape == (0,) and res["cols"].shape == (90,)
    with pytest.raises(ValueError):
        sc.dense_round(POINT[:-1])


def test_scorer_pool_step_dict():
    sc = _scorer()
    d = sc._lib.pool
    dtypes = dict(leave=np.int64, enter=np.int64, dropped=np.int64, enter_indptr=np.int32, enter_indices=np.int32, enter_values=np.float64,
                  enter_rhs=np.float64, enter_sense=np.int32, enter_key=np.float64)
    scalars = dict(n_in_lp=40, n_parked=6, n_violated=5, n_dropped=1)
    res = sc.pool_step(POINT, max_age=2, max_return=9)                 # copy=True is the default here
    assert sc._lib.calls[-1] == ("pool_step", 1e-9, 1e-6, 2, 10, 9)
    assert set(res) == set(dtypes) | set(scalars) and sc._pool_rows == 49 and sc.round_count == 0
    _check_arrays(res, d, dtypes)
    assert all(res[k] == v and type(res[k]) is int for k, v in scalars.items())
    views = sc.pool_step(POINT, copy=False)
    again = sc.pool_step(POINT, copy=False)
    assert all(np.array_equal(again[k], views[k]) and again[k].ctypes.data == views[k].ctypes.data for k in dtypes)
    d["enter_values"][:] += 1.0
    assert np.array_equal(views["enter_values"], d["enter_values"]) and np.array_equal(res["enter_values"], d["enter_values"] - 1.0)
    sc._lib.empty = True
    res = sc.pool_step()
    assert all(res[k].shape == (0,) and res[k].dtype == dtypes[k] for k in dtypes if k != "enter_indptr")
    assert res["enter_indptr"].tolist() == [0] and res["enter_indptr"].dtype == np.int32 and res["n_violated"] == 0
    with pytest.raises(ValueError):
        sc.pool_step(POINT[:-1])
    with pytest.raises(ValueError):
        sc.pool_step(POINT, max_age=0)
    sc._h = None
    with pytest.raises(_capi.SdpCutError, match="closed"):
        sc.pool_step(POINT)
