"""Cut pool on the device (sdpcut_pool_*; csrc/pool.hip) against its numpy twin (sdpcutsel_via_nn_amd/cutpool.py), bit for bit:
the whole state (pool_state) and every field of a step's result.  The twin restates the device's arithmetic operation by
operation, so nothing here has a tolerance.

Scenario of the size tests (n = 20, 230 LP columns): rows of 2..20 entries, both senses, right-hand sides placed relative to the
sequentially summed activity at a base point: exactly on it (d == 0), slack or violated by 0.1 ||row||, slack or violated by
0.001 ||row||.  The steps' points are the base point (step 1) and perturbations of it by 0.01, so the last two kinds change sides
from step to step; max_age = drop_age = 2 and a small max_return keep every class moving: from the fourth step on rows leave,
return, stay parked and drop in every step (asserted on the twin for the sizes >= 63)."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INST = os.path.join(ROOT, "tests", "golden", "instances", "spar020-100-1.in")
N = 20
NCOLS = N * (N + 1) // 2 + N
STATE = ("serial", "state", "age", "nnz", "sense", "rhs", "norm", "cols", "vals")
OUT = ("leave", "enter", "dropped", "enter_indptr", "enter_indices", "enter_values", "enter_rhs", "enter_sense", "enter_key")
COUNTS = ("n_in_lp", "n_parked", "n_violated", "n_dropped")


@pytest.fixture(scope="module")
def sc():
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import harness
    s = pkg.Scorer(0)
    inst = harness.parse_boxqp(INST)
    s.set_instance(N, np.asarray(inst["Q_arr"], dtype=np.float64))
    s.inst = inst
    yield s
    s.close()


def same_state(sc, tw):
    a, b = sc.pool_state(), tw.pool_state()
    assert a["n"] == b["n"] and a["next_serial"] == b["next_serial"]
    for f in STATE:
        assert a[f].dtype == b[f].dtype and np.array_equal(a[f], b[f]), f
    return a


def same_step(sc, tw, point, **par):
    a, b = sc.pool_step(point, **par), tw.pool_step(point, **par)
    for f in OUT:
        assert a[f].dtype == b[f].dtype and np.array_equal(a[f], b[f]), (f, a[f][:8], b[f][:8])
    for f in COUNTS:
        assert a[f] == b[f], f
    same_state(sc, tw)
    return b


def block(rng, m, base):
    """m rows as CSR arrays; the right-hand side of row i sits relative to its activity at ``base`` by the kind i % 5"""
    from sdpcutsel_via_nn_amd.cutpool import row_norm
    ptr, ind, val, rhs, sense = [0], [], [], [], []
    for i in range(m):
        ln = 2 + i % 19                                             # 2 .. 20
        cols = rng.choice(NCOLS, size=ln, replace=False)
        vals = rng.standard_normal(ln)
        sg = 1 if rng.random() < 0.5 else -1
        act = 0.0
        for c, v in zip(cols, vals):
            act = act + float(v) * float(base[c])
        shift = (0.0, 0.1, -0.1, 0.001, -0.001)[i % 5] * row_norm(vals, ln)      # d at the base point
        ind.extend(cols)
        val.extend(vals)
        ptr.append(len(ind))
        rhs.append(act - sg * shift if shift else act)
        sense.append(sg)
    return (np.array(ptr, np.int32), np.array(ind, np.int32), np.array(val), np.array(rhs), np.array(sense, np.int32))


def scenario(P, seed=3):
    """('add', block) / ('step', point) operations: P rows first, six steps, smaller blocks in between"""
    rng = np.random.default_rng(seed + P)
    base = rng.random(NCOLS)
    ops = [("add", block(rng, P, base))]
    for t in range(6):
        ops.append(("step", base if t == 0 else base + 0.01 * rng.standard_normal(NCOLS)))
        if t < 5:
            ops.append(("add", block(rng, P // 8 + 5, base)))
    return ops


# ------------------------------------------------------------------------------------------ 1. device against twin
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 4097])
def test_device_equals_twin_bit_for_bit(sc, P):
    from sdpcutsel_via_nn_amd.cutpool import CutPoolTwin, check_step, row_distance
    cap = 2 * P + 64
    sc.pool_create(cap)
    tw = CutPoolTwin(cap, NCOLS)
    par = dict(tight_tol=1e-9, viol_tol=1e-6, max_age=2, drop_age=2, max_return=P // 16 + 1)
    step_no, capped = 0, False
    for op in scenario(P):
        if op[0] == "add":
            assert sc.pool_add(*op[1]) == tw.pool_add(*op[1])
            same_state(sc, tw)
            continue
        step_no += 1
        before = tw.pool_state()
        if step_no == 1:      # the exact zeros are there: rows whose sequentially summed distance at the base point is 0.0
            d = [row_distance(before["cols"][r], before["vals"][r], before["nnz"][r], before["rhs"][r], before["sense"][r], op[1])
                 for r in range(before["n"])]
            assert sum(1 for x in d if x == 0.0) >= (P + 4) // 5
        out = same_step(sc, tw, op[1], **par)
        assert check_step(before, par, op[1], out, tw.pool_state())
        if P >= 63 and step_no >= 4:      # every class is populated
            assert out["leave"].size and out["enter"].size and out["dropped"].size and out["n_parked"]
        capped = capped or out["n_violated"] > out["enter"].size
    assert step_no == 6 and (capped or P < 257)      # max_return did cut the list of violated rows
    if P >= 63:
        assert set(before["nnz"].tolist()) == set(range(2, 21)) and set(before["sense"].tolist()) == {1, -1}


# ------------------------------------------------------------------------------------------ 2. ties
def test_ties_enter_by_ascending_serial(sc):
    from sdpcutsel_via_nn_amd.cutpool import CutPoolTwin
    sc.pool_create(64)
    tw = CutPoolTwin(64, NCOLS)
    one = ([3, 7], [3.0, 4.0], 1.0)                                 # 3 x3 + 4 x7 >= 1, norm 5
    rows = [([1], [1.0], 0.25)] + [one] * 3 + [([2, 4], [1.0, 1.0], 0.5)] + [one] * 4
    ptr = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int32)
    blk = (ptr, np.concatenate([r[0] for r in rows]).astype(np.int32), np.concatenate([r[1] for r in rows]), np.array([r[2] for r in rows]), None)
    assert sc.pool_add(*blk) == tw.pool_add(*blk) == 0
    slack, viol = np.ones(NCOLS), np.zeros(NCOLS)
    viol[2] = viol[4] = -4.0                                        # row 4: key 8.5 / sqrt 2 beats the copies' 1 / 5
    par = dict(tight_tol=1e-9, viol_tol=1e-6, max_age=1, drop_age=9)
    o = same_step(sc, tw, slack, max_return=0, **par)
    assert o["leave"].size == 9
    o = same_step(sc, tw, viol, max_return=4, **par)                # the cap falls inside the group of seven copies
    assert o["n_violated"] == 9 and list(o["enter"]) == [4, 0, 1, 2]
    assert o["enter_key"][1] == 0.25 and np.all(o["enter_key"][2:] == 0.2)
    o = same_step(sc, tw, viol, max_return=3, **par)
    assert list(o["enter"]) == [3, 5, 6]                            # the lower serials of the remaining copies


# ------------------------------------------------------------------------------------------ 3. compaction
PATTERNS = {"none": lambda n: np.zeros(n, bool), "all": lambda n: np.ones(n, bool),
            "first": lambda n: np.arange(n) == 0, "last": lambda n: np.arange(n) == n - 1,
            "alternating": lambda n: np.arange(n) % 2 == 0,
            "run_over_a_workgroup_boundary": lambda n: (np.arange(n) >= 250) & (np.arange(n) < 263)}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_compaction_patterns(sc, pattern):
    from sdpcutsel_via_nn_amd.cutpool import CutPoolTwin
    n = 600                                                          # three workgroups of 256 rows
    drop = PATTERNS[pattern](n)
    sc.pool_create(n + 3)
    tw = CutPoolTwin(n + 3, NCOLS)
    # row i: x0 + m_i x1 + (i + 1) x2 >= 0.5; m_i = 0 for the rows to drop.  At (1, 0, 0) all are slack, at (1, -1, 0) the rows with
    # m_i = 1 are violated and return, the others stay parked and drop
    ptr = np.arange(n + 1, dtype=np.int32) * 3
    ind = np.tile(np.array([0, 1, 2], np.int32), n)
    val = np.stack([np.ones(n), np.where(drop, 0.0, 1.0), np.arange(1, n + 1, dtype=np.float64)], 1).reshape(-1)
    blk = (ptr, ind, val, np.full(n, 0.5), None)
    assert sc.pool_add(*blk) == tw.pool_add(*blk) == 0
    a, b = np.zeros(NCOLS), np.zeros(NCOLS)
    a[0] = b[0] = 1.0
    b[1] = -1.0
    par = dict(tight_tol=1e-9, viol_tol=1e-6, max_age=1, drop_age=1)
    o = same_step(sc, tw, a, max_return=n, **par)
    assert o["leave"].size == n and o["n_parked"] == n
    o = same_step(sc, tw, b, max_return=n, **par)
    assert np.array_equal(o["dropped"], np.flatnonzero(drop)) and o["enter"].size == n - drop.sum()
    st = same_state(sc, tw)
    assert np.array_equal(st["serial"], np.flatnonzero(~drop)) and np.array_equal(st["vals"][:, 2], np.flatnonzero(~drop) + 1.0)
    # the pool goes on working in the arrays it was compacted into
    if drop.any():
        more = (ptr[:4], ind[:9], val[:9], np.full(3, 0.5), None)
        assert sc.pool_add(*more) == tw.pool_add(*more) == n
        same_step(sc, tw, a, max_return=n, **par)


# ------------------------------------------------------------------------------------------ 4. edge cases
def test_edge_cases_and_refusals(sc):
    from sdpcutsel_via_nn_amd import _capi
    from sdpcutsel_via_nn_amd.cutpool import CutPoolTwin
    sc.pool_create(8)
    tw = CutPoolTwin(8, NCOLS)
    par = dict(tight_tol=1e-9, viol_tol=1e-6, max_age=1, drop_age=3)
    pt = np.ones(NCOLS)
    o = same_step(sc, tw, pt, max_return=4, **par)                   # a step on an empty pool
    assert o["n_in_lp"] == o["n_parked"] == 0 and o["leave"].size == 0
    rows = (np.array([0, 1, 3, 4, 5, 6], np.int32), np.array([0, 1, 2, 3, 4, 5], np.int32), np.ones(6), np.array([0.5, 9.0, 0.5, 0.5, 0.5]), None)
    assert sc.pool_add(*rows) == tw.pool_add(*rows) == 0
    o = same_step(sc, tw, pt, max_return=4, **dict(par, max_age=5))  # a step with nothing parked
    assert o["n_parked"] == 0 and o["enter"].size == 0
    o = same_step(sc, tw, pt, max_return=0, **par)                   # the slack rows are parked (row 1 is violated and stays)
    assert list(o["leave"]) == [0, 2, 3, 4]
    o = same_step(sc, tw, np.zeros(NCOLS), max_return=0, **par)      # max_return = 0: all four are violated, none returns
    assert o["n_violated"] == 4 and o["enter"].size == 0 and o["n_parked"] == 4
    before = same_state(sc, tw)
    # refusals of the Python layer ...
    for bad in ((np.array([0, 1], np.int32), np.array([NCOLS], np.int32), np.ones(1), np.zeros(1), None),         # a bad column
                (np.arange(5, dtype=np.int32), np.zeros(4, np.int32), np.ones(4), np.zeros(4), None)):             # beyond the capacity
        with pytest.raises(ValueError):
            sc.pool_add(*bad)
    # ... and of the library itself, reached past the Python checks
    i32, f64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)

    def raw_add(ptr, ind, val, rhs):
        first = ctypes.c_int64(-7)
        ptr, ind = np.asarray(ptr, np.int32), np.asarray(ind, np.int32)
        val, rhs = np.asarray(val, np.float64), np.asarray(rhs, np.float64)
        return sc._lib.sdpcut_pool_add_csr(sc._h, rhs.shape[0], ptr.ctypes.data_as(i32), ind.ctypes.data_as(i32), val.ctypes.data_as(f64),
                                           rhs.ctypes.data_as(f64), None, ctypes.byref(first))
    assert raw_add([0, 1, 2, 3, 4], [0, 0, 0, 0], [1.0] * 4, [0.0] * 4) == -1         # beyond the capacity (5 + 4 > 8)
    assert raw_add([0, 1], [NCOLS], [1.0], [0.0]) == -1 and raw_add([0, 1], [-1], [1.0], [0.0]) == -1
    assert raw_add([0, 0], [], [], [0.0]) == -1 and raw_add([0, 21], [0] * 21, [1.0] * 21, [0.0]) == -1
    assert raw_add([0, 1], [0], [float("nan")], [0.0]) == -1 and raw_add([0, 1], [0], [1.0], [float("inf")]) == -1
    after = same_state(sc, tw)
    assert all(np.array_equal(before[f], after[f]) for f in STATE) and after["next_serial"] == before["next_serial"]
    par_c = _capi.PoolParams(1e-9, 1e-6, 0, 3, 0)
    assert sc._lib.sdpcut_pool_step(sc._h, None, ctypes.byref(par_c), ctypes.byref(_capi.PoolStep())) == -1
    # step, add and step again after the errors
    same_step(sc, tw, np.zeros(NCOLS), max_return=2, **par)
    rows2 = (np.array([0, 2], np.int32), np.array([7, 8], np.int32), np.array([1.0, -1.0]), np.array([0.0]), np.array([-1], np.int32))
    assert sc.pool_add(*rows2) == tw.pool_add(*rows2) == 5
    same_step(sc, tw, pt, max_return=2, **par)
    same_step(sc, tw, None, max_return=8, **par)                     # the current point again


# ------------------------------------------------------------------------------------------ 5. real rows
def test_real_round_rows(sc):
    from sdpcutsel_via_nn_amd import harness
    from sdpcutsel_via_nn_amd.cutpool import CutPoolTwin
    p7, p8 = (harness.random_mccormick_point(N, np.random.default_rng(s)) for s in (7, 8))
    assert sc.set_candidates_cover(sc.inst["adj"], 3) > 500
    r = sc.round_csr(1, 300, point=p7, copy=True)
    m = int(r["rhs"].shape[0])
    assert 50 < m <= 300
    sc.pool_create(512)
    tw = CutPoolTwin(512, NCOLS)
    blk = (r["indptr"], r["indices"], r["values"], r["rhs"], None)
    assert sc.pool_add(*blk) == tw.pool_add(*blk) == 0
    par = dict(tight_tol=1e-9, viol_tol=1e-6, max_age=1, drop_age=4)
    o = same_step(sc, tw, p8, max_return=50, **par)
    assert 0 < o["leave"].size < m                                   # at another point some of the cuts are slack, some still cut
    o = same_step(sc, tw, p7, max_return=50, **par)                  # every cut cuts off the point it was made at
    assert o["n_violated"] > 0 and o["enter"].size == min(50, o["n_violated"])
    # the handle's round still works next to the pool, with the point the step left
    r2 = sc.round_csr(1, 300, point=None, copy=True)
    for f in ("idx", "score", "indptr", "indices", "values", "rhs"):
        assert np.array_equal(r[f], r2[f]), f


# ------------------------------------------------------------------------------------------ 6. the loop
def test_cut_select_algo_with_the_pool():
    import sdpcutsel_via_nn_amd as pkg
    plain = pkg.CutSolver()
    b0 = plain.cut_select_algo(INST, 3, 0.1, strat=1, nb_rounds_cuts=5)[0]
    off = pkg.CutSolver()
    b1 = off.cut_select_algo(INST, 3, 0.1, strat=1, nb_rounds_cuts=5, pool_max_age=None)[0]
    assert b1 == b0 and getattr(off, "pool_log", None) is None       # the default is today's path
    cs = pkg.CutSolver()
    seen = []

    def on_round(r, log):
        lp = cs._my_prob
        loop = getattr(cs, "pool_loop", None)
        seen.append((lp.linear_constraints.get_num(), None if loop is None else loop.row_serial.copy(), np.array(lp.get_values())))
    res = cs.cut_select_algo(INST, 3, 0.1, strat=1, nb_rounds_cuts=5, pool_max_age=2, on_round=on_round)
    b, sdp, n_cand = res[0], res[4], res[6]
    quota = pkg.CutSolver.selection_size(0.1, n_cand)
    assert b[0] == b0[0] and len(b) == 6 and len(cs.pool_log) == 5
    better = np.sign(b0[-1] - b0[0])
    for r in range(1, 6):
        assert (b[r] - b[r - 1]) * better >= -1e-7 * abs(b[r - 1]), (r, b)
    loop = cs.pool_loop
    model_rows = int(np.sum(loop.row_serial < 0))
    st = cs._agg_list.scorer.pool_state()
    pos = {int(s): i for i, s in enumerate(st["serial"])}
    assert sum(rec["leave"] for rec in cs.pool_log) > 0
    for r, rec in enumerate(cs.pool_log):
        rows_at_solve, _, point = seen[r]                            # the LP that was solved before round r + 1
        assert rec["lp_rows"] == rows_at_solve and rec["added"] == sdp[r + 1] <= quota
        if r:
            prev = cs.pool_log[r - 1]
            assert rows_at_solve == model_rows + prev["in_lp"] + prev["added"]
            assert rec["in_lp"] + rec["parked"] + sum(q["dropped"] for q in cs.pool_log[:r + 1]) == sum(q["added"] for q in cs.pool_log[:r])
    # every leaving row was slack and every entering row violated at its point: recomputed with numpy from the rows the pool holds
    # (a dropped row has left the arrays: the run's drop_age of 10 keeps all of them)
    assert all(rec["dropped"] == 0 for rec in cs.pool_log)
    steps = loop.steps
    assert len(steps) == 5
    for (point, out) in steps:
        for s in out["leave"]:
            i = pos[int(s)]
            ln = st["nnz"][i]
            d = st["sense"][i] * (np.dot(st["vals"][i, :ln], point[st["cols"][i, :ln]]) - st["rhs"][i])
            assert d > 1e-9 * st["norm"][i] * (1 - 1e-6)
        for s in out["enter"]:
            i = pos[int(s)]
            ln = st["nnz"][i]
            d = st["sense"][i] * (np.dot(st["vals"][i, :ln], point[st["cols"][i, :ln]]) - st["rhs"][i])
            assert -d > 1e-6 * st["norm"][i] * (1 - 1e-6)
