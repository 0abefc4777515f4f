"""Cut pool, the parts that need no device: the numpy twin step by step on a hand-built pool, random sequences through the
invariant checker, row deletion on both LP paths, a tiny cutting-plane loop with the twin pool, the new names of the C-ABI and the
argument checks of the Python layer."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")
NAMES = ("sdpcut_pool_create", "sdpcut_pool_destroy", "sdpcut_pool_add_csr", "sdpcut_pool_step", "sdpcut_pool_get")


def csr(rows):
    """[(cols, vals, rhs, sense)] -> (indptr, indices, values, rhs, sense)"""
    ptr = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int32)
    return (ptr, np.concatenate([r[0] for r in rows]).astype(np.int32), np.concatenate([r[1] for r in rows]).astype(np.float64),
            np.array([r[2] for r in rows], dtype=np.float64), np.array([r[3] for r in rows], dtype=np.int32))


# ------------------------------------------------------------------------------------------ the twin, transition by transition
def test_twin_on_a_hand_built_pool():
    from sdpcutsel_via_nn_amd.cutpool import CutPoolTwin
    G, L = 1, -1
    rows = [([0], [1.0], 0.5, G),            # 0: x0 >= 0.5
            ([1], [2.0], 4.0, G),            # 1: 2 x1 >= 4, norm 2
            ([2], [1.0], 5.0, L),            # 2: x2 <= 5
            ([3], [1.0], 4.5, G),            # 3: x3 >= 4.5
            ([0, 1], [3.0, 4.0], 1.0, G),    # 4: 3 x0 + 4 x1 >= 1, norm 5
            ([4], [1.0], 0.5, L),            # 5: x4 <= 0.5
            ([5], [1.0], 0.0, G),            # 6: x5 >= 0
            ([2, 3], [1.0, 1.0], 7.0, L)]    # 7: x2 + x3 <= 7
    tw = CutPoolTwin(16, 6)
    assert tw.pool_add(*csr(rows)) == 0
    st = tw.pool_state()
    assert st["n"] == 8 and list(st["serial"]) == list(range(8)) and st["norm"][4] == 5.0 and st["norm"][1] == 2.0
    par = dict(tight_tol=1e-9, viol_tol=0.0, max_age=2, drop_age=2, max_return=8)
    p1 = np.array([1.0, 2.0, 3.0, 4.0, 0.5, 0.25])
    # d: 0.5, 0 (exact), 2, -0.5, 10, 0 (exact), 0.25, 0 (exact)
    o = tw.pool_step(p1, **par)
    assert o["leave"].size == o["enter"].size == o["dropped"].size == 0 and o["n_in_lp"] == 8 and o["n_parked"] == 0
    assert list(tw.age) == [1, 0, 1, 0, 1, 0, 1, 0]           # slack rows age; d == 0 and violated rows are not slack
    # tight resets the age: row 0 is tight at the second point, row 6 stays slack
    p2 = p1.copy()
    p2[0] = 0.5
    o = tw.pool_step(p2, **par)
    assert list(o["leave"]) == [2, 4, 6] and o["n_in_lp"] == 5 and o["n_parked"] == 3
    assert list(tw.state) == [0, 0, 1, 0, 1, 0, 1, 0] and list(tw.age) == [0] * 8
    # parked -> in: rows 4 and 6 are violated at p3 (keys 9.5 / 5 = 1.9 and 1.0), row 2 is satisfied with d == 0 exactly
    p3 = np.array([-1.5, -1.0, 5.0, 4.0, 0.5, -1.0])
    o = tw.pool_step(p3, **dict(par, max_return=1))
    assert o["n_violated"] == 2 and list(o["enter"]) == [4] and o["enter_key"][0] == 9.5 / 5.0
    assert list(o["enter_indptr"]) == [0, 2] and list(o["enter_indices"]) == [0, 1] and list(o["enter_values"]) == [3.0, 4.0]
    assert o["enter_rhs"][0] == 1.0 and o["enter_sense"][0] == 1 and o["dropped"].size == 0
    assert list(tw.state) == [0, 0, 1, 0, 0, 0, 1, 0] and tw.age[2] == 1 and tw.age[6] == 1 and tw.age[4] == 0
    # parked -> dropped: nothing returns (max_return 0), rows 2 and 6 reach drop_age and the arrays close up
    o = tw.pool_step(p3, **dict(par, max_return=0))
    assert o["n_violated"] == 1 and o["enter"].size == 0 and list(o["dropped"]) == [2, 6] and o["n_dropped"] == 2
    assert list(tw.serial) == [0, 1, 3, 4, 5, 7] and o["n_parked"] == 0 and o["n_in_lp"] == 6
    # serials are never reused
    assert tw.pool_add(*csr(rows[:1])) == 8 and tw.pool_state()["next_serial"] == 9
    # a row parked by a step is not examined as parked in that step: with max_age 1 row 8 (x0 >= 0.5, slack at p1) is parked
    # at once, keeps age 0 and cannot return or age as a parked row before the next step
    o = tw.pool_step(p1, **dict(par, max_age=1, drop_age=1, max_return=4))
    assert 8 in o["leave"] and o["enter"].size == 0 and o["dropped"].size == 0
    assert tw.state[list(tw.serial).index(8)] == 1 and tw.age[list(tw.serial).index(8)] == 0


def test_twin_refuses_bad_blocks_and_stays_unchanged():
    from sdpcutsel_via_nn_amd.cutpool import CutPoolTwin
    tw = CutPoolTwin(3, 6)
    tw.pool_add(*csr([([0], [1.0], 0.0, 1)]))
    before = tw.pool_state()
    bad = [csr([([0], [1.0], 0.0, 1)] * 3),                                   # beyond the capacity
           csr([([6], [1.0], 0.0, 1)]), csr([([-1], [1.0], 0.0, 1)]),         # column outside the LP
           csr([([0], [np.nan], 0.0, 1)]), csr([([0], [1.0], np.inf, 1)]),    # not finite
           csr([(list(range(6)) * 4, [1.0] * 24, 0.0, 1)]),                   # longer than 20
           (np.array([0, 0]), np.zeros(0, np.int32), np.zeros(0), np.zeros(1), None),      # an empty row
           csr([([0], [1.0], 0.0, 2)])]                                       # a sense that is none
    for blk in bad:
        with pytest.raises(ValueError):
            tw.pool_add(*blk)
        after = tw.pool_state()
        assert all(np.array_equal(before[k], after[k]) for k in before)
    with pytest.raises(ValueError):
        CutPoolTwin(0, 6)
    with pytest.raises(ValueError):
        CutPoolTwin(4194305, 6)
    for kw in (dict(max_age=0), dict(drop_age=0), dict(max_return=-1), dict(tight_tol=-1.0), dict(viol_tol=float("nan")), dict(max_age=1.5)):
        with pytest.raises(ValueError):
            tw.pool_step(np.zeros(6), **kw)


def random_rows(rng, m, ncols):
    rows = []
    for _ in range(m):
        ln = int(rng.integers(1, 21))
        cols = rng.choice(ncols, size=min(ln, ncols), replace=False)
        vals = rng.standard_normal(cols.shape[0])
        rows.append((cols, vals, float(rng.standard_normal() * 0.3), int(rng.choice([1, -1]))))
    return rows


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_sequences_keep_the_invariants(seed):
    from sdpcutsel_via_nn_amd.cutpool import CutPoolTwin, check_step
    rng = np.random.default_rng(seed)
    ncols = 30
    tw = CutPoolTwin(600, ncols)
    ever, gone, parked_seen, entered = set(), set(), False, 0
    for step in range(12):
        m = int(rng.integers(0, 40))
        if m:
            s0 = tw.pool_add(*csr(random_rows(rng, m, ncols)))
            ever |= set(range(s0, s0 + m))
        par = dict(tight_tol=1e-9, viol_tol=1e-6, max_age=int(rng.integers(1, 4)), drop_age=int(rng.integers(1, 5)),
                   max_return=int(rng.integers(0, 12)))
        pt = rng.random(ncols)
        before = tw.pool_state()
        out = tw.pool_step(pt, **par)
        after = tw.pool_state()
        assert check_step(before, par, pt, out, after)
        gone |= set(int(s) for s in out["dropped"])
        live = set(int(s) for s in after["serial"])
        assert live | gone == ever and not (live & gone)          # every serial ever added: in the LP, parked or dropped
        parked_seen = parked_seen or bool(np.any(after["state"] == 1))
        entered += int(out["enter"].size)
    assert gone and parked_seen and entered                       # the sequences did reach every class


def test_check_step_catches_a_wrong_order():
    from sdpcutsel_via_nn_amd.cutpool import CutPoolTwin, check_step
    tw = CutPoolTwin(8, 2)
    tw.pool_add(*csr([([0], [1.0], 1.0, 1), ([0], [1.0], 2.0, 1), ([0], [1.0], 3.0, 1)]))
    tw.state[:] = 1
    par = dict(tight_tol=1e-9, viol_tol=1e-6, max_age=2, drop_age=9, max_return=2)
    before = tw.pool_state()
    out = tw.pool_step(np.zeros(2), **par)
    after = tw.pool_state()
    assert list(out["enter"]) == [2, 1] and check_step(before, par, np.zeros(2), out, after)
    swapped = dict(out, enter=out["enter"][::-1].copy(), enter_key=out["enter_key"][::-1].copy(), enter_rhs=out["enter_rhs"][::-1].copy())
    with pytest.raises(AssertionError):
        check_step(before, par, np.zeros(2), swapped, after)


# ------------------------------------------------------------------------------------------ deleting rows of the LP
def random_lp(rng, nv=12, m=60):
    from sdpcutsel_via_nn_amd import harness
    A = rng.standard_normal((m, nv))
    x0 = rng.random(nv)
    b = A @ x0 - rng.random(m) * 0.5          # A x >= b holds at x0 with slack up to 0.5
    c = rng.standard_normal(nv)
    return A, b, c


def fill(lp, A, b, rows):
    nv = A.shape[1]
    ptr = np.arange(len(rows) + 1, dtype=np.int64) * nv
    lp.linear_constraints.add_csr(ptr, np.tile(np.arange(nv), len(rows)), A[rows].reshape(-1).copy(), b[rows].copy(), "G")


@pytest.mark.parametrize("incremental", [True, False])
def test_delete_rows_keeps_the_optimum_and_the_model_consistent(incremental):
    from scipy.optimize import linprog
    from sdpcutsel_via_nn_amd import harness
    rng = np.random.default_rng(5)
    A, b, c = random_lp(rng)
    lp = harness.LinearRelaxation(c, incremental=incremental)      # (without SciPy's HiGHS binding both cases run the fallback)
    fill(lp, A, b, list(range(40)))
    lp.solve()
    obj0, x = lp.get_objective_value(), lp.get_values()
    slack = np.flatnonzero(A[:40] @ x - b[:40] > 1e-7)
    assert 0 < slack.size < 40
    lp.delete_rows(slack[::-1])               # any order
    assert lp.linear_constraints.get_num() == 40 - slack.size
    lp.solve()
    assert abs(lp.get_objective_value() - obj0) <= 1e-9 * max(1.0, abs(obj0))
    # rows added after a deletion, and a deletion that spans rows HiGHS holds and rows it does not hold yet
    fill(lp, A, b, list(range(40, 60)))
    kept = [r for r in range(40) if r not in set(slack.tolist())] + list(range(40, 60))
    drop_pos = [0, len(kept) - 1]
    lp.delete_rows(drop_pos)
    kept = [r for i, r in enumerate(kept) if i not in drop_pos]
    lp.solve()
    if lp._core is not None:
        assert lp._rows_passed == lp.linear_constraints.get_num() == len(kept)
    ref = linprog(c, A_ub=-A[kept], b_ub=-b[kept], bounds=(0, 1), method="highs-ds")
    assert ref.status == 0 and abs(lp.get_objective_value() - ref.fun) <= 1e-9 * max(1.0, abs(ref.fun))
    assert np.array_equal(lp.linear_constraints.rhs_from(0), b[kept]) and set(lp.linear_constraints.senses) == {"G"}
    with pytest.raises(ValueError):
        lp.delete_rows([1, 1])
    with pytest.raises(IndexError):
        lp.delete_rows([len(kept)])


def test_row_store_delete_rows_over_mixed_blocks():
    from sdpcutsel_via_nn_amd import harness
    st = harness._RowStore()
    st.add(lin_expr=[harness.SparsePair([0, 1], [1.0, 2.0]), harness.SparsePair([2], [3.0])], rhs=[1.0, 2.0], senses=["G", "L"])
    st.add_csr(np.array([0, 1, 3]), np.array([4, 5, 6]), np.array([7.0, 8.0, 9.0]), np.array([3.0, 4.0]), "G")
    st.add(lin_expr=[], rhs=[], senses=[])
    st.delete_rows([1, 2])
    assert st.get_num() == 2 and st.rhs == [1.0, 4.0] and st.senses == ["G", "G"]
    data, cols, lens = st.csr_parts()
    assert list(data) == [1.0, 2.0, 8.0, 9.0] and list(cols) == [0, 1, 5, 6] and list(lens) == [2, 2]
    assert [r.ind for r in st.rows] == [[0, 1], [5, 6]]
    st.delete_rows([])
    assert st.get_num() == 2


# ------------------------------------------------------------------------------------------ a tiny loop with the twin pool
def test_tiny_loop_with_the_twin_pool_keeps_bounds_monotone():
    from sdpcutsel_via_nn_amd import harness
    from sdpcutsel_via_nn_amd.cutpool import CutPoolTwin, PoolLoop
    rng = np.random.default_rng(12)      # (an instance whose McCormick optimum is not PSD: lambda_min -1.28)
    n = 8
    L = n * (n + 1) // 2
    Q = rng.integers(-50, 51, size=(n, n)).astype(np.float64)
    Q = np.triu(Q) + np.triu(Q, 1).T
    half = Q.copy()
    half[np.diag_indices(n)] /= 2.0
    inst = dict(nb_vars=n, nb_lifted=L, c=rng.integers(-50, 51, size=n).astype(np.float64), Q_arr=half[np.triu_indices(n)],
                adj=np.ones((n, n), bool))
    xd = np.array([n * i - i * (i - 1) // 2 for i in range(n)])
    triples = list(itertools.combinations(range(n), 3))
    max_age = 2

    def run(pooled):
        lp = harness.boxqp_relaxation(inst)
        model_rows = lp.linear_constraints.get_num()
        loop = PoolLoop(lp, CutPoolTwin(4096, L + n), max_age, drop_age=3) if pooled else None
        seen = []

        def separate(round_no, point):
            if loop:
                assert lp.linear_constraints.get_num() == loop.row_serial.shape[0]
                loop.step(point, 10)
                st = loop.pool.pool_state()
                assert np.all(st["age"][st["state"] == 0] < max_age)          # no LP row is as old as max_age at a solve
                seen.append((loop.log[-1], int(np.sum(loop.row_serial >= 0)), model_rows))
            cuts = []
            for t in triples:
                cols_x = [L + i for i in t]
                cols_X = [xd[t[a]] + (t[b] - t[a]) for a in range(3) for b in range(a, 3)]
                M = np.zeros((4, 4))
                M[0, 0] = 1.0
                M[0, 1:] = M[1:, 0] = point[cols_x]
                for (a, b), col in zip([(a, b) for a in range(3) for b in range(a, 3)], cols_X):
                    M[1 + a, 1 + b] = M[1 + b, 1 + a] = point[col]
                lam, V = np.linalg.eigh(M)
                if lam[0] < -1e-7:
                    v = V[:, 0]
                    coef = [2 * v[0] * v[1 + a] for a in range(3)] + [(1 if a == b else 2) * v[1 + a] * v[1 + b] for a in range(3) for b in range(a, 3)]
                    cuts.append((lam[0], cols_x + cols_X, coef, -v[0] * v[0]))
            cuts.sort(key=lambda c: c[0])
            cuts = cuts[:10]
            if cuts:
                ptr = np.arange(len(cuts) + 1, dtype=np.int64) * 9
                lp.linear_constraints.add_csr(ptr, np.concatenate([c[1] for c in cuts]).astype(np.int64),
                                              np.concatenate([c[2] for c in cuts]), np.array([c[3] for c in cuts]), "G")
            if loop:
                assert loop.adopt() == len(cuts)
            return {"sdp": len(cuts)}
        return harness.run_cut_rounds(lp, separate, 8), loop, seen

    log, loop, seen = run(True)
    b = log.bounds
    assert len(b) == 9 and b[-1] > b[0]
    for r in range(1, len(b)):
        assert b[r] >= b[r - 1] - 1e-7 * abs(b[r - 1]), (r, b)
    assert sum(rec["leave"] for rec in loop.log) > 0                # the pool did something
    for rec, pooled_rows, model_rows in seen:
        assert rec["in_lp"] == pooled_rows                          # the pool's LP rows are the LP's rows that carry a serial
    for prev, rec in zip(loop.log, loop.log[1:]):
        assert rec["lp_rows"] == seen[0][2] + prev["in_lp"] + prev["added"]
    st = loop.pool.pool_state()
    assert sorted(st["serial"][st["state"] == 0].tolist()) == sorted(loop.row_serial[loop.row_serial >= 0].tolist())
    plain, _, _ = run(False)
    assert plain.bounds[0] == b[0]


# ------------------------------------------------------------------------------------------ the C-ABI's new names
def test_new_names_in_header_binding_and_export_map():
    from sdpcutsel_via_nn_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "sdpcut.h")).read()
    declared = set(re.findall(r"^(?:int|const char \*)\s*(sdpcut_\w+)\s*\(", hdr, flags=re.M))
    exports = open(os.path.join(CSRC, "exports.map")).read()
    pats = re.findall(r"global:\s*([^;]+);", exports)
    for name in NAMES:
        assert name in declared and name in _capi.SIGNATURES
        assert pats and any(re.fullmatch(p.strip().replace("*", r"\w*"), name) for p in pats)
    assert int(re.search(r"#define SDPCUT_POOL_MAX_ROWS (\d+)", hdr).group(1)) == 4194304 == _capi.POOL_MAX_ROWS
    assert "pool.hip" in __import__("sdpcutsel_via_nn_amd.build", fromlist=["SOURCES"]).SOURCES
    assert [n for n, _ in _capi.PoolParams._fields_] == ["tight_tol", "viol_tol", "max_age", "drop_age", "max_return"]
    assert ctypes.sizeof(_capi.PoolParams) == 32 and ctypes.sizeof(_capi.PoolStep) == 7 * 8 + 9 * 8
    assert "sdpcut_pool_params_t" in hdr and "sdpcut_pool_step_t" in hdr
    for m in ("pool_create", "pool_add", "pool_step", "pool_state"):
        assert callable(getattr(_capi.Scorer, m))


def test_argument_checks_of_the_python_layer():
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import _capi
    assert _capi.check_pool_params(1e-9, 1e-6, 2, 10, 0) == (1e-9, 1e-6, 2, 10, 0)
    for bad in ((-1e-9, 1e-6, 2, 10, 0), (1e-9, float("inf"), 2, 10, 0), (1e-9, 1e-6, 0, 10, 0), (1e-9, 1e-6, 2, 0, 0),
                (1e-9, 1e-6, 2, 10, -1), (1e-9, 1e-6, 2.5, 10, 0)):
        with pytest.raises(ValueError):
            _capi.check_pool_params(*bad)
    # the solver's front door: refused before anything touches a device or a file
    cs = pkg.CutSolver()
    with pytest.raises(AssertionError, match="strategy 0"):
        cs.cut_select_algo("no-such-file.in", 3, 0.1, strat=0, pool_max_age=2)
    with pytest.raises(ValueError, match="max_age"):
        cs.cut_select_algo("no-such-file.in", 3, 0.1, strat=1, pool_max_age=0)
    with pytest.raises(ValueError, match="drop_age"):
        cs.cut_select_algo("no-such-file.in", 3, 0.1, strat=1, pool_max_age=2, pool_drop_age=0)
    with pytest.raises(ValueError, match="max_return"):
        cs.cut_select_algo("no-such-file.in", 3, 0.1, strat=1, pool_max_age=2, pool_return=-1)
    with pytest.raises(ValueError, match="tol"):
        cs.cut_select_algo("no-such-file.in", 3, 0.1, strat=1, pool_max_age=2, pool_viol_tol=-1.0)
    # without pool_max_age the other pool arguments are not even looked at: today's path
    with pytest.raises((OSError, IOError)):
        cs.cut_select_algo("no-such-file.in", 3, 0.1, strat=1, pool_drop_age=0)
