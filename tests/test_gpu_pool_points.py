"""The pool at tree nodes on the device (sdpcut_pool_separate_points, sdpcut_pool_drop; csrc/pool_points.hip) against its numpy twin
(sdpcutsel_via_nn_amd/cutpool.py), byte for byte: every array of every point, the counts, and the pool's state.  The twin restates
the device's arithmetic operation by operation, so nothing here has a tolerance.  The pools are tests/pool_points_cases.py: keys
under direct control (one-entry rows whose right-hand side IS the key) and mixed pools of real row shapes."""
import ctypes

import numpy as np
import pytest

import pool_points_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import harness
    s = pkg.Scorer(0)
    inst = harness.parse_boxqp(pc.INST)
    s.set_instance(pc.N, np.asarray(inst["Q_arr"], dtype=np.float64))
    s.inst = inst
    yield s
    s.close()


def pair(sc, cap):
    from sdpcutsel_via_nn_amd.cutpool import CutPoolTwin
    sc.pool_create(cap)
    return CutPoolTwin(cap, pc.NCOLS)


def both(sc, tw, points, max_return, **kw):
    """the call on the device and on the twin, equal byte for byte, the pool untouched -> (twin's result, select_passes per point)"""
    before = sc.pool_state()
    a = sc.pool_separate_points(points, max_return, **kw)
    passes = pc.same_separation(a, tw.pool_separate_points(np.asarray(points), max_return, **kw))
    pc.same_state(sc.pool_state(), before)
    pc.same_state(before, tw.pool_state())
    return a, passes


# ------------------------------------------------------------------------------------------ 1. sizes, points, caps, masks
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 5000, 12000])
def test_device_equals_twin_over_sizes(sc, n):
    from sdpcutsel_via_nn_amd.cutpool import check_separation
    tw = pair(sc, n + 8)
    base, rng = pc.mixed_pool([sc, tw], n)
    st = pc.same_state(sc.pool_state(), tw.pool_state())
    if n >= 63:
        assert set(st["state"].tolist()) == {0, 1} and set(st["nnz"].tolist()) == set(pc.LENGTHS) and set(st["sense"].tolist()) == {1, -1}
    seen = selected = 0
    combos = ((0, "all"), (1, "parked"), (7, "lp"), (4096, "all"), (7, "all"), (4096, "parked"), (4096, "lp"))
    for P in (1, 2, 7) if n > 65 else (1, 2, 7, 256):
        pts = pc.points_near(rng, base, P)
        wide = np.full((P, pc.NCOLS + 5), np.nan)      # point_ld larger than the points: what lies between them is never read
        wide[:, :pc.NCOLS] = pts
        for mr, states in combos:
            if P == 256 and mr == 4096 and states != "all":
                continue
            out, passes = both(sc, tw, wide[:, :pc.NCOLS] if mr == 7 else pts, mr, states=states)
            assert passes == [8 * (o["n_violated"] > pc.LIST and mr > 0) for o in out]
            selected += sum(p > 0 for p in passes)
            seen += sum(o["n_violated"] for o in out)
            if P in (2, 7) and mr == 7:
                assert check_separation(st, pts, 1e-6, states, mr, out)
    assert seen > 0 or n == 1
    # about half the rows of a mixed pool are violated near the base point: the 12 000 rows (a size of this file's own) take
    # the radix select with rows of real lengths and keys that differ in every byte, the other sizes never do
    assert (selected > 0) == (n == 12000)


# ------------------------------------------------------------------------------------------ 2. keys under direct control
def controlled(sc, keys, viol_tol=0.0):
    tw = pair(sc, len(keys))
    blk = pc.single_rows(keys)
    assert sc.pool_add(*blk) == tw.pool_add(*blk) == 0
    return tw


@pytest.mark.parametrize("m", [pc.LIST, 5000])
@pytest.mark.parametrize("b", range(8))
def test_byte_families_through_and_past_the_list(sc, b, m):
    """m = 5000 violated rows exceed the list of 4096 and force the radix select; m = 4096 still fit it.  The keys differ in byte b
    alone, so digit 7 - b of the select decides alone; with 128 or 256 byte values every key has copies, the threshold's ties too"""
    keys = pc.byte_family(b, m)
    tw = controlled(sc, keys)
    pts = np.stack([pc.zero_point(), pc.zero_point()])
    order = sorted((-k, i) for i, k in enumerate(keys))
    for mr in (1, 7, 4096):
        out, passes = both(sc, tw, pts, mr, viol_tol=0.0)
        assert all(p > 0 for p in passes) if m > pc.LIST else passes == [0, 0]
        for o in out:      # the keys ARE the right-hand sides: the expected order needs no arithmetic
            assert o["n_violated"] == m and list(o["serial"]) == [i for _, i in order[:mr]] and list(o["key"]) == [-k for k, _ in order[:mr]]
    out, passes = both(sc, tw, pts, 0, viol_tol=0.0)
    assert [o["n_violated"] for o in out] == [m, m] and all(o["serial"].size == 0 for o in out)


@pytest.mark.parametrize("m", [pc.LIST, 5000])
def test_identical_rows_return_the_lowest_serials(sc, m):
    tw = controlled(sc, pc.identical(m))
    pts = pc.zero_point()[None, :]
    for mr in (1, 7, 4096):
        out, passes = both(sc, tw, pts, mr)
        assert (passes[0] > 0) == (m > pc.LIST)
        assert out[0]["n_violated"] == m and np.array_equal(out[0]["serial"], np.arange(mr)) and np.all(out[0]["key"] == 0.75)
    # after the lowest serials have gone the next ones come back
    assert sc.pool_drop(np.arange(0, 10)) == tw.pool_drop(np.arange(0, 10)) == 10
    out, _ = both(sc, tw, pts, 3)
    assert list(out[0]["serial"]) == [10, 11, 12]


def test_tie_runs_inf_keys_and_thresholds(sc):
    z = pc.zero_point()[None, :]
    tw = controlled(sc, pc.tie_runs())
    for mr in (4, 7, 12, 13, 4096):
        out, _ = both(sc, tw, z, mr)
    assert list(out[0]["serial"][-5:]) == [1, 5, 10, 14, 17]
    out, _ = both(sc, tw, z, 7)
    assert list(out[0]["serial"]) == [2, 7, 13, 0, 3, 4, 6]
    tw = pair(sc, 16)
    blk, nv = pc.inf_keys()
    assert sc.pool_add(*blk) == tw.pool_add(*blk) == 0
    out, _ = both(sc, tw, z, 4096, viol_tol=0.0)
    assert out[0]["n_violated"] == nv and list(out[0]["serial"]) == [1, 5, 3, 0] and list(out[0]["key"]) == [np.inf, np.inf, 1e300, 5.0]
    for vt in (1e-6, 0.0):
        tw = controlled(sc, pc.threshold(vt))
        out, _ = both(sc, tw, z, 4096, viol_tol=vt)
        assert out[0]["n_violated"] == 3 and list(out[0]["serial"]) == [0, 3, 6] and np.all(out[0]["key"] == np.nextafter(vt, np.inf))


def test_real_rows(sc):
    """rows the device's own separations made on spar020-100-1 (3, 4, 6, 9, 14 and 20 entries), both senses, both states"""
    blk, pt = pc.real_rows(sc, sc.inst)
    assert set(np.diff(blk[0]).tolist()) == {3, 4, 6, 9, 14, 20}
    tw = pair(sc, 512)
    assert sc.pool_add(*blk) == tw.pool_add(*blk) == 0
    from sdpcutsel_via_nn_amd import harness
    other = harness.random_mccormick_point(pc.N, np.random.default_rng(8))
    pc.park_some([sc, tw], other)
    st = pc.same_state(sc.pool_state(), tw.pool_state())
    assert set(st["state"].tolist()) == {0, 1}
    pts = np.stack([pt, other, 0.5 * (pt + other)])
    res = {states: both(sc, tw, pts, 25, states=states)[0] for states in ("all", "parked", "lp")}
    assert res["all"][0]["n_violated"] > 25      # every cut cuts off the point it was made at
    assert all(res["all"][p]["n_violated"] == res["parked"][p]["n_violated"] + res["lp"][p]["n_violated"] for p in range(3))


# ------------------------------------------------------------------------------------------ 3. nothing changes
def test_handle_point_and_rounds_are_untouched(sc):
    """the handle's point, scores and a NULL-point round after the call give the bytes of a handle that never made it"""
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import harness
    p7, p8 = (harness.random_mccormick_point(pc.N, np.random.default_rng(s)) for s in (7, 8))
    fresh = pkg.Scorer(0)
    try:
        res = []
        for s, sep in ((sc, True), (fresh, False)):
            s.set_instance(pc.N, np.asarray(sc.inst["Q_arr"], dtype=np.float64))
            s.set_candidates_cover(sc.inst["adj"], 3)
            r = s.round_csr(1, 100, point=p7, copy=True)
            if sep:
                s.pool_create(256)
                s.pool_add(r["indptr"], r["indices"], r["values"], r["rhs"])
                o = s.pool_separate_points(np.stack([p8, p7]), 50, copy=True)
                assert o[1]["n_violated"] > 0 and o[1]["serial"].size == min(50, o[1]["n_violated"])
            res.append((r, s.round_csr(1, 100, point=None, copy=True)))
        for f in ("idx", "score", "indptr", "indices", "values", "rhs"):
            assert res[0][0][f].tobytes() == res[0][1][f].tobytes() == res[1][1][f].tobytes(), f
        # ... and a pool step that keeps the current point (point=None) steps at p7, not at a point of the separation
        from sdpcutsel_via_nn_amd.cutpool import CutPoolTwin
        tw = CutPoolTwin(256, pc.NCOLS)
        r = res[0][0]
        tw.pool_add(r["indptr"], r["indices"], r["values"], r["rhs"])
        par = dict(tight_tol=1e-9, viol_tol=1e-6, max_age=1, drop_age=5, max_return=10)
        a, b = sc.pool_step(None, **par), tw.pool_step(p7, **par)
        assert all(np.array_equal(a[f], b[f]) for f in ("leave", "enter", "dropped", "enter_key")) and a["n_violated"] == b["n_violated"]
    finally:
        fresh.close()
        sc.set_instance(pc.N, np.asarray(sc.inst["Q_arr"], dtype=np.float64))      # (the module's handle as the other tests expect it)


def test_steps_interleaved_with_separations_equal_the_uninterrupted_sequence(sc):
    from sdpcutsel_via_nn_amd.cutpool import CutPoolTwin
    tw = pair(sc, 700)                       # the twin runs the steps alone
    rng = np.random.default_rng(11)
    base = rng.random(pc.NCOLS)
    par = dict(tight_tol=1e-9, viol_tol=1e-6, max_age=2, drop_age=2, max_return=9)
    moved = dict(leave=0, enter=0, dropped=0)
    for t in range(6):
        blk = pc.mixed_block(rng, 90, base)
        assert sc.pool_add(*blk) == tw.pool_add(*blk)
        pts = pc.points_near(rng, base, 3)
        sc.pool_separate_points(pts, 20)                                # between add and step
        a, b = sc.pool_step(pts[0], **par), tw.pool_step(pts[0], **par)
        for f in ("leave", "enter", "dropped", "enter_indptr", "enter_indices", "enter_values", "enter_rhs", "enter_sense", "enter_key"):
            assert a[f].tobytes() == b[f].tobytes(), (t, f)
        for f in moved:
            moved[f] += int(b[f].size)
        sc.pool_separate_points(pts[1:], 4096, states="parked")           # between step and add
        pc.same_state(sc.pool_state(), tw.pool_state())
    assert all(moved.values()), moved      # rows left, returned and dropped between the separations


# ------------------------------------------------------------------------------------------ 4. pool_drop
PATTERNS = {"none": lambda n: np.zeros(n, bool), "all": lambda n: np.ones(n, bool),
            "first": lambda n: np.arange(n) == 0, "last": lambda n: np.arange(n) == n - 1,
            "alternating": lambda n: np.arange(n) % 2 == 0,
            "run_over_a_workgroup_boundary": lambda n: (np.arange(n) >= 250) & (np.arange(n) < 263),
            "unknown_serials": None, "duplicates": None}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_drop_patterns(sc, pattern):
    n = 600                                                          # three workgroups of 256 rows
    tw = pair(sc, n + 8)
    base, rng = pc.mixed_pool([sc, tw], n)
    st = pc.same_state(sc.pool_state(), tw.pool_state())
    if pattern == "unknown_serials":
        ser, want = np.array([-3, n, n + 100, 2 ** 40], dtype=np.int64), 0
    elif pattern == "duplicates":
        ser, want = np.array([599, 17, 17, 0, 599, 300, 17, -1], dtype=np.int64), 4
    else:
        ser = st["serial"][PATTERNS[pattern](n)][::-1].copy()          # (descending: the call sorts)
        want = int(ser.size)
    assert sc.pool_drop(ser) == tw.pool_drop(ser) == want
    after = pc.same_state(sc.pool_state(), tw.pool_state())
    assert after["n"] == n - want and not np.isin(after["serial"], ser).any() and after["next_serial"] == n
    pts = pc.points_near(rng, base, 2)
    if after["n"]:
        both(sc, tw, pts, 40)
    # the pool goes on working in the arrays it was compacted into: add, step (rows leave, return and drop), separate, drop again
    blk = pc.mixed_block(rng, 7, base)
    assert sc.pool_add(*blk) == tw.pool_add(*blk) == n
    par = dict(tight_tol=1e-9, viol_tol=1e-6, max_age=1, drop_age=2, max_return=15)
    for v in pts:
        a, b = sc.pool_step(v, **par), tw.pool_step(v, **par)
        for f in ("leave", "enter", "dropped", "enter_key", "enter_indices", "enter_values"):
            assert a[f].tobytes() == b[f].tobytes(), f
        assert (a["n_in_lp"], a["n_parked"]) == (b["n_in_lp"], b["n_parked"])      # (the counts the drop kept right)
        pc.same_state(sc.pool_state(), tw.pool_state())
    both(sc, tw, pts, 4096)
    left = sc.pool_state()["serial"]
    assert sc.pool_drop(left[1::3]) == tw.pool_drop(left[1::3]) == left[1::3].size
    pc.same_state(sc.pool_state(), tw.pool_state())
    assert sc._pool_rows == tw.n


# ------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(sc):
    from sdpcutsel_via_nn_amd import _capi
    import sdpcutsel_via_nn_amd as pkg
    lib, h = sc._lib, sc._h
    dp = ctypes.POINTER(ctypes.c_double)
    pts = np.zeros((2, pc.NCOLS))
    out = (_capi.PoolSep * 256)()

    def call(P=2, points=pts, ld=pc.NCOLS, mask=3, vt=1e-6, mr=4, o=out):
        return lib.sdpcut_pool_separate_points(h, P, None if points is None else points.ctypes.data_as(dp), ld, mask, vt, mr, o)

    def msg():
        return lib.sdpcut_last_error(h).decode()
    sc.pool_destroy()
    assert call() == -4 and "sdpcut_pool_create first" in msg()                                         # no pool (SDPCUT_ESTATE)
    gone = ctypes.c_int64(-1)
    assert lib.sdpcut_pool_drop(h, 0, None, ctypes.byref(gone)) == -4
    tw = pair(sc, 6000)
    blk = pc.single_rows(pc.identical(5000))
    assert sc.pool_add(*blk) == tw.pool_add(*blk) == 0
    before = sc.pool_state()
    assert call() == 0 and out[1].n_violated == 5000 and out[1].n_rows == 4 and out[1].select_passes == 8
    for kw, text in ((dict(P=0), "n_points"), (dict(P=257), "n_points"), (dict(ld=pc.NCOLS - 1), "point_ld"), (dict(points=None), "points is NULL"),
                     (dict(o=None), "out is NULL"), (dict(mask=0), "state_mask"), (dict(mask=4), "state_mask"), (dict(mask=7), "state_mask"),
                     (dict(vt=-1.0), "viol_tol"), (dict(vt=float("nan")), "viol_tol"), (dict(vt=float("inf")), "viol_tol"),
                     (dict(mr=-1), "max_return"), (dict(mr=4097), "max_return")):
        assert call(**kw) == -1 and text in msg(), kw
    big = np.zeros((256, pc.NCOLS))
    assert call(P=256, points=big, mr=4096) == -1                                                       # 256 x 1 114 240 bytes > 256 MiB
    assert "256 points x 1114240 bytes" in msg() and "285245440 bytes exceeds the limit of 268435456 bytes" in msg()
    with pytest.raises(ValueError, match="exceeds the limit of 268435456 bytes"):
        sc.pool_separate_points(big, 4096)
    assert call(P=240, points=big, mr=4096) == 0 and out[239].n_violated == 5000 and out[239].n_rows == 4096
    assert lib.sdpcut_pool_drop(h, -1, None, None) == -1 and lib.sdpcut_pool_drop(h, 2, None, None) == -1
    assert lib.sdpcut_pool_drop(h, 0, None, ctypes.byref(gone)) == 0 and gone.value == 0               # n = 0 is fine
    # a pending round refuses both calls
    sc.set_candidates_cover(sc.inst["adj"], 3)
    from sdpcutsel_via_nn_amd import harness
    assert lib.sdpcut_round_csr_begin(h, harness.random_mccormick_point(pc.N, np.random.default_rng(7)).ctypes.data_as(dp), 1, 20) == 0
    assert call() == -4 and "pending" in msg()
    assert lib.sdpcut_pool_drop(h, 0, None, None) == -4
    assert lib.sdpcut_round_csr_end(h, ctypes.byref(_capi.RoundCsr())) == 0
    pc.same_state(sc.pool_state(), before)
    both(sc, tw, pts, 5)
    # a pool made for another nb_vars
    other = pkg.Scorer(0)
    try:
        other.set_instance(pc.N, np.asarray(sc.inst["Q_arr"], dtype=np.float64))
        other.pool_create(4)
        other.set_instance(5, np.zeros(15))
        with pytest.raises(pkg.SdpCutError, match="instance changed"):
            other.pool_separate_points(np.zeros((1, 20)), 1)
        with pytest.raises(pkg.SdpCutError, match="instance changed"):
            other.pool_drop([0])
    finally:
        other.close()
    # an empty pool returns zeros for every point
    sc.pool_create(4)
    o = sc.pool_separate_points(pts, 4)
    assert all(x["n_violated"] == 0 and x["serial"].size == 0 and list(x["indptr"]) == [0] and x["select_passes"] == 0 for x in o)
    assert sc.pool_drop([0, 1]) == 0


# ------------------------------------------------------------------------------------------ 6. the loop
def test_root_pool_separates_at_child_nodes():
    """A root run leaves its eigen-cuts in the pool; two children of a branching ask it at their LP points (solved WITHOUT the
    run's cuts).  Every returned row is violated at its point, valid at rank-one points of the cube, and does not lower a child's
    bound."""
    import sdpcutsel_via_nn_amd as pkg
    from sdpcutsel_via_nn_amd import harness
    cs = pkg.CutSolver()
    cs.cut_select_algo(pc.INST, 3, 0.1, strat=1, nb_rounds_cuts=4, pool_max_age=2)
    root = np.array(cs._my_prob.get_values())
    inst = harness.parse_boxqp(pc.INST)
    n, L = pc.N, pc.N * (pc.N + 1) // 2
    j = int(np.argmin(np.abs(root[L:] - 0.5)))                        # the most fractional variable
    rng = np.random.default_rng(5)
    xs = rng.random((64, n))
    iu = np.triu_indices(n)
    rank_one = np.concatenate([xs[:, iu[0]] * xs[:, iu[1]], xs], axis=1)      # (x x^T packed | x)
    lps, pts, bounds = [], [], []
    for lo, hi in ((0.0, 0.5), (0.5, 1.0)):
        lb, ub = np.zeros(n), np.ones(n)
        lb[j], ub[j] = lo, hi
        lp = harness.boxqp_relaxation(inst, lb, ub)
        lp.solve()
        lps.append(lp)
        pts.append(np.array(lp.get_values()))
        bounds.append(lp.get_objective_value())
    state_before = cs.pool_loop.pool.pool_state()
    res = cs.separate_pool_points(np.stack(pts), 50)
    pc.same_state(cs.pool_loop.pool.pool_state(), state_before)
    assert len(res) == 2 and sum(r[3] for r in res) > 0
    for lp, v, bound, (csr, sense, serials, n_viol) in zip(lps, pts, bounds, res):
        ptr, ind, val, rhs = csr
        assert rhs.shape[0] == min(50, n_viol) == serials.shape[0] == sense.shape[0]
        for r in range(rhs.shape[0]):
            c, a = ind[ptr[r]:ptr[r + 1]], val[ptr[r]:ptr[r + 1]]
            nr = np.sqrt(np.sum(a * a))
            assert -sense[r] * (np.dot(a, v[c]) - rhs[r]) > 1e-6 * nr * (1 - 1e-6)               # violated at its point
            assert np.all(sense[r] * (rank_one[:, c] @ a - rhs[r]) >= -1e-9 * nr)                # (v0 + v.x)^2 >= 0 at every rank-one point
        if rhs.shape[0]:
            flip = np.repeat(sense, np.diff(ptr)).astype(np.float64)
            lp.linear_constraints.add_csr(np.array(ptr, dtype=np.int64), np.array(ind), val * flip, rhs * sense, "G")
            lp.solve()
            assert lp.get_objective_value() - bound >= -1e-7 * max(1.0, abs(bound))
