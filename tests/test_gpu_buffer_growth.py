"""The buffers behind the calls that take many LP points ("Buffers"): every one grows on demand and is never
shrunk, so what a call returns must not depend on how large an earlier call left them.  One handle runs each of the seven calls
over a ladder of batch sizes that grows, shrinks and grows again -- and over a ladder of the size that drives its result block --
and every result is compared, byte for byte, with the same call on a handle made for it.  The shapes are the smallest at which a
stride taken from a capacity instead of P, a stale size or a lost zero-fill shows: list A of tests/op_sequences.py (130 candidates
of four variables, the one-launch route), n = 40.

The second half holds the refusals the seven calls share (csrc/common.h: check_point_batch, check_box_pair): each, alone, gives
the code and the text the call gave before the intake was shared -- the table below was copied from those sources."""
import ctypes

import numpy as np
import pytest

import op_sequences as seq

pytestmark = pytest.mark.gpu

LADDER = (1, 4, 2, 9, 3)
POOL_CAP = 64
M = seq.L_VARS + seq.N_VARS


class _Model(seq.Model):
    def __init__(self):
        seq.Model.__init__(self)
        self.lst, self.tri = "A", True


@pytest.fixture(scope="module")
def fx():
    f = seq.Fixtures()
    # Nine LP points for list A: the fixture's gen, strong and weak points and six blends of them (the McCormick set is convex).
    # None of them makes a selection of list A declare itself void, so no point is redone by the single-point round (asserted
    # below through SDPCUT_STAT_POINTS_REDONE); the fixture's `mid` and `psd` points -- exact ties, nothing violated -- are left out
    # for that reason.
    g, s, w = f.point("gen"), f.point("strong"), f.point("weak")
    f.nine = np.stack([g, s, w, 0.5 * (g + s), 0.5 * (g + w), 0.5 * (s + w), 0.25 * g + 0.75 * s, 0.75 * g + 0.25 * w, (g + s + w) / 3.0])
    f.boxes9 = np.stack([np.stack(f.box(seed)) for seed in range(1, 10)])      # [9, 2, n]
    f.objective = np.random.default_rng(5).normal(size=M)
    # the rows x_i - X_ii of the fixture's pool block, entered as "L" rows: violated wherever X_ii < x_i
    f.pool_sense = -np.ones(f.pool_block[3].shape[0], dtype=np.int32)
    return f


def _handle(fx):
    import sdpcutsel_via_nn_amd as pkg
    sc = seq.new_handle(pkg, fx, _Model())
    sc.set_objective(fx.objective)
    sc.pool_create(POOL_CAP)
    sc.pool_add(*fx.pool_block, sense=fx.pool_sense)
    return sc


@pytest.fixture(scope="module")
def grown(fx):
    sc = _handle(fx)
    yield sc
    sc.close()


def _same(a, b, where):
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), where
        for k in a:
            _same(a[k], b[k], "%s.%s" % (where, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (where, i))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    else:
        assert a == b, where


def _stats(sc):
    from sdpcutsel_via_nn_amd import _capi
    return {k: sc.get_stat(getattr(_capi, "STAT_" + k)) for k in ("POINTS_REDONE", "DIVERSE_POINTS_FAST", "TRI_POINTS_FAST", "NODE_EVAL_POINTS")}


# name -> (call(scorer, points, boxes or None, size), takes boxes, the statistic that counts its fast points or None).  `size` is
# what drives the result block: sel_size of the rounds, max_out of the triangle rounds, max_return of the separation.
CALLS = {
    "score_points": (lambda sc, pts, bx, size: sc.score_points(pts, boxes=bx), True, None),
    "round_csr_points": (lambda sc, pts, bx, size: sc.round_csr_points(pts, 4, size, copy=True, boxes=bx), True, None),
    "round_csr_points_diverse": (lambda sc, pts, bx, size: sc.round_csr_points_diverse(pts, 2, size, 0.5, copy=True, boxes=bx), True,
                                 "DIVERSE_POINTS_FAST"),
    "efficacy_points": (lambda sc, pts, bx, size: sc.efficacy_points(pts), False, None),
    "tri_round_csr_points": (lambda sc, pts, bx, size: sc.tri_round_csr_points(pts, size, boxes=bx, copy=True), True, "TRI_POINTS_FAST"),
    "pool_separate_points": (lambda sc, pts, bx, size: sc.pool_separate_points(pts, size, copy=True), False, None),
    "node_eval_points": (lambda sc, pts, bx, size: sc.node_eval_points(pts, boxes=bx, copy=True), True, "NODE_EVAL_POINTS"),
}
DEFAULT_SIZE = {"round_csr_points": 50, "round_csr_points_diverse": 20, "tri_round_csr_points": 300, "pool_separate_points": 6}
SIZE_LADDER = {"round_csr_points": (10, 100, 10), "round_csr_points_diverse": (10, 100, 10), "tri_round_csr_points": (8, 4096, 8),
               "pool_separate_points": (4, 512, 4)}
VARIANTS = [(name, boxed) for name in CALLS for boxed in ((False, True) if CALLS[name][1] else (False,))]


def _against_fresh(fx, grown, name, boxed, P, size, first):
    """the call on the long-lived handle and on a handle made for it: equal byte for byte, by the fast route"""
    call, _, fast = CALLS[name]
    pts = np.ascontiguousarray(fx.nine[first:first + P])
    bx = np.ascontiguousarray(fx.boxes9[first:first + P]) if boxed else None
    before = _stats(grown)
    got = call(grown, pts, bx, size)
    after = _stats(grown)
    fresh = _handle(fx)
    try:
        want = call(fresh, pts, bx, size)
        fresh_stats = _stats(fresh)
    finally:
        fresh.close()
    where = "%s%s P=%d size=%s" % (name, " boxed" if boxed else "", P, size)
    _same(got, want, where)
    assert after["POINTS_REDONE"] == before["POINTS_REDONE"] and fresh_stats["POINTS_REDONE"] == 0, where
    if fast:
        assert after[fast] - before[fast] == P and fresh_stats[fast] == P, where
    return got


@pytest.mark.parametrize("name, boxed", VARIANTS, ids=["%s%s" % (n, "-boxed" if b else "") for n, b in VARIANTS])
def test_ladder_of_batch_sizes(fx, grown, name, boxed):
    for step, P in enumerate(LADDER):
        # (another window of the nine points at every step: a row left over from the step before is not the row asked for)
        got = _against_fresh(fx, grown, name, boxed, P, DEFAULT_SIZE.get(name, 0), first=(2 * step) % (10 - P))
        if name == "pool_separate_points":
            assert all(o["n_violated"] > 0 and o["serial"].size > 0 for o in got)      # the comparison is not one of empty arrays
        if name == "tri_round_csr_points" and not boxed:
            assert any(v.size for o in got for v in o.values() if isinstance(v, np.ndarray))


@pytest.mark.parametrize("name, boxed", [v for v in VARIANTS if v[0] in SIZE_LADDER],
                         ids=["%s%s" % (n, "-boxed" if b else "") for n, b in VARIANTS if n in SIZE_LADDER])
def test_ladder_of_result_sizes(fx, grown, name, boxed):
    for size in SIZE_LADDER[name]:
        _against_fresh(fx, grown, name, boxed, 3, size, first=1)


# ------------------------------------------------------------------------------------------ the shared refusals
EINVAL = -1
NE = "sdpcut_node_eval_points: "
N_POINTS = "n_points must be 1 .. SDPCUT_BATCH_MAX_POINTS (256)"
# entry point -> the text of (n_points out of range, points NULL, point_ld too small, one of lb / ub NULL); None: the call takes no
# boxes.  Copied from points.hip, tri_points.hip, pool_points.hip and node_eval.hip as they were before the intake was shared.
REFUSALS = {
    "sdpcut_score_points": (N_POINTS, "points is NULL", "point_ld must be at least L + n", None),
    "sdpcut_score_points_boxed": (N_POINTS, "points is NULL", "point_ld must be at least L + n", "sdpcut_score_points_boxed: lb or ub is NULL"),
    "sdpcut_round_csr_points": (N_POINTS, "points is NULL", "point_ld must be at least L + n", None),
    "sdpcut_round_csr_points_boxed": (N_POINTS, "points is NULL", "point_ld must be at least L + n",
                                      "sdpcut_round_csr_points_boxed: lb or ub is NULL"),
    "sdpcut_round_csr_points_diverse": (N_POINTS, "points is NULL", "point_ld must be at least L + n",
                                        "sdpcut_round_csr_points_diverse: lb or ub is NULL"),
    "sdpcut_efficacy_points": (N_POINTS, "points is NULL", "point_ld must be at least L + n", None),
    "sdpcut_tri_round_csr_points": (N_POINTS, "points is NULL", "point_ld must be at least L + n",
                                    "sdpcut_tri_round_csr_points: lb and ub must both be given or both be NULL"),
    "sdpcut_pool_separate_points": (N_POINTS, "points is NULL", "point_ld must be at least L + n", None),
    "sdpcut_node_eval_points": (NE + N_POINTS, NE + "points is NULL", NE + "point_ld must be at least L + n",
                                NE + "lb and ub must both be given or both be NULL"),
}


@pytest.mark.parametrize("entry", sorted(REFUSALS))
def test_shared_refusals_keep_code_and_text(fx, grown, entry):
    from sdpcutsel_via_nn_amd import _capi
    lib, h = grown._lib, grown._h
    dp = ctypes.POINTER(ctypes.c_double)
    n, N = seq.N_VARS, seq.LIST_LENGTHS["A"]
    pts = np.ascontiguousarray(fx.nine[:2])
    lo, hi = np.ascontiguousarray(fx.boxes9[:2, 0]), np.ascontiguousarray(fx.boxes9[:2, 1])
    a, b, c = np.empty((2, N)), np.empty((2, N)), np.empty((2, N))
    rounds, infos = (_capi.RoundCsr * 2)(), (_capi.DiverseInfo * 2)()

    def ptr(x):
        return None if x is None else x.ctypes.data_as(dp)

    def call(P=2, points=pts, ld=M, lb=lo, ub=hi):
        p, l, u = ptr(points), ptr(lb), ptr(ub)
        return {
            "sdpcut_score_points": lambda: lib.sdpcut_score_points(h, P, p, ld, _capi.EIG | _capi.NN, ptr(a), ptr(b)),
            "sdpcut_score_points_boxed": lambda: lib.sdpcut_score_points_boxed(h, P, p, ld, l, u, n, _capi.EIG | _capi.NN, ptr(a), ptr(b)),
            "sdpcut_round_csr_points": lambda: lib.sdpcut_round_csr_points(h, P, p, ld, 4, 20, rounds),
            "sdpcut_round_csr_points_boxed": lambda: lib.sdpcut_round_csr_points_boxed(h, P, p, ld, l, u, n, 4, 20, rounds),
            "sdpcut_round_csr_points_diverse": lambda: lib.sdpcut_round_csr_points_diverse(h, P, p, ld, l, u, n, 2, 20, 80, 0.5, rounds, infos),
            "sdpcut_efficacy_points": lambda: lib.sdpcut_efficacy_points(h, P, p, ld, ptr(a), ptr(b), ptr(c)),
            "sdpcut_tri_round_csr_points": lambda: lib.sdpcut_tri_round_csr_points(h, P, p, ld, l, u, 100, (_capi.TriCsr * 2)()),
            "sdpcut_pool_separate_points": lambda: lib.sdpcut_pool_separate_points(h, P, p, ld, 3, 1e-6, 4, (_capi.PoolSep * 2)()),
            "sdpcut_node_eval_points": lambda: lib.sdpcut_node_eval_points(h, P, p, ld, l, u, 10, 1, 0.2, (_capi.NodeEval * 2)()),
        }[entry]()

    def refused(text, **kw):
        assert call(**kw) == EINVAL and lib.sdpcut_last_error(h).decode() == text, (entry, kw, lib.sdpcut_last_error(h).decode())

    assert call() == 0, lib.sdpcut_last_error(h).decode()      # nothing wrong: the call is served
    n_points, null_points, short_ld, half_box = REFUSALS[entry]
    refused(n_points, P=0)
    refused(n_points, P=257)
    refused(null_points, points=None)
    refused(short_ld, ld=M - 1)
    if half_box is not None:
        refused(half_box, ub=None)
        refused(half_box, lb=None)
    assert call() == 0, lib.sdpcut_last_error(h).decode()      # the handle stays usable
