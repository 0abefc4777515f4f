"""The one driver of the batched rounds (csrc/points.hip: round_points) with the verdicts of a point in the SAME batch: answered,
answered with an empty head, answered after its assembly went round again.  The other suites reach these paths one per batch; what
a merged driver can get wrong is their order inside one call: the relaunch of the `again` points, then csr_out_from_block over
every slice, then the redone points over theirs.

List: the dim-3 cover of spar020-100-1 (1051 candidates), the smallest shipped list whose head spans two assembly workgroups (only
an assembly of more than 64 entries has a look-back to give up).  Batch of four points: a generic McCormick point, the PSD point
X = x x^T (nothing violated: an empty head under strategy 1), the McCormick vertex of test_gpu_batch_points.py::
test_structured_points, a second generic point.  Shapes of the L5 give-up cases (tests/giveup_cases.py): plain strategy 1, sel 129;
filtered strategy 1, sel 80, pool 320, max_parallel 1.  Each without boxes and with a box per point (strategy 1 reads none; the
per-point calls still set theirs).  One give-up of the look-back is injected into the batch's assembly launch
(SDPCUT_OPT_INJECT_GIVEUP, the suite's mechanism; nothing faults).

Premise, measured and not assumed: whether the vertex is redone through the single-point call depends on its tie groups
(test_structured_points allows 0 to 3 redone points).  At the commit before the driver, at these exact inputs, the injected batch
moves SDPCUT_STAT_POINTS_REDONE by 0 in all four cases (heads 129, 0, 129, 129 plain and 80, 0, 80, 80 filtered; three fallbacks,
one injection), and so does the undisturbed batch: REDONE_BEFORE, asserted below.  So no point of this batch is redone, and the
order "redone points after the `again` points" is held only by test_gpu_batch_points.py::test_structured_points and
test_gpu_diverse_points.py::test_vertex_point_in_a_batch."""
import os

import numpy as np
import pytest

import giveup_cases as gc

pytestmark = pytest.mark.gpu

ARRAYS = ("idx", "score", "lam", "ks", "set_inds", "row_entry", "indptr", "indices", "values", "rhs")
PLAIN, FILTERED = dict(strat=1, sel=129), dict(strat=1, sel=80, pool=320)
PSD = 1      # row of the batch
REDONE_BEFORE = 0      # SDPCUT_STAT_POINTS_REDONE delta of the batch before the driver existed, all four cases (see above)


def batch_points():
    """-> [4, L + n]"""
    from sdpcutsel_via_nn_amd import harness
    inp = gc.inputs("spar020")
    n = inp["n"]
    L = n * (n + 1) // 2
    inst = harness.parse_boxqp(os.path.join(gc.GOLDEN, "instances", "spar020-100-1.in"))
    lp = harness.boxqp_relaxation(inst)
    lp.solve()
    vertex = np.array(lp.get_values(), dtype=np.float64)
    vertex[L:] = 0.5
    x = np.random.default_rng(5).uniform(0.0, 1.0, n)
    psd = np.concatenate([(x[:, None] * x[None, :])[np.triu_indices(n)], x])
    g = [harness.random_mccormick_point(n, np.random.default_rng(s)) for s in (5000, 5001)]
    return np.stack([g[0], psd, vertex, g[1]])


def batch_boxes(n):
    import nodebox_cases as nc
    return np.stack([np.stack((np.zeros(n), np.ones(n)))] + [np.stack(nc.random_box(n, 900 + p)) for p in range(1, 4)])


def run_batch(sc, pts, filtered, boxes):
    if filtered:
        return sc.round_csr_points_diverse(pts, FILTERED["strat"], FILTERED["sel"], 1.0, pool_size=FILTERED["pool"], copy=True, boxes=boxes)
    return sc.round_csr_points(pts, PLAIN["strat"], PLAIN["sel"], copy=True, boxes=boxes)


def run_single(sc, point, filtered, box=None):
    if box is not None:
        sc.set_box(box[0], box[1])
    try:
        if filtered:
            return sc.round_csr_diverse(point, FILTERED["strat"], FILTERED["sel"], 1.0, pool_size=FILTERED["pool"], copy=True)
        return sc.round_csr(PLAIN["strat"], PLAIN["sel"], point=point, copy=True)
    finally:
        if box is not None:
            sc.clear_box()


def assert_same_round(got, want, what=""):
    """every field of a round, floating-point arrays as bit patterns; `info` where the round is a filtered one"""
    assert set(got) == set(want), what
    for f in ARRAYS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
        assert got[f].tobytes() == want[f].tobytes(), (what, f)
    assert (got["n_total"], got["new_strat"], got["counters"]) == (want["n_total"], want["new_strat"], want["counters"]), what
    assert got.get("info") == want.get("info"), what


def moved(sc, before=None):
    from sdpcutsel_via_nn_amd import _capi
    now = {"injected": sc.get_stat(_capi.STAT_INJECTED), "fallbacks": sc.get_stat(_capi.STAT_SELECT_FALLBACKS),
           "redone": sc.get_stat(_capi.STAT_POINTS_REDONE)}
    return now if before is None else {k: now[k] - before[k] for k in now}


def injected_batch(sc, pts, filtered, boxes):
    """arm one give-up of the look-back, run the batch -> (rounds, what the statistics moved by)"""
    from sdpcutsel_via_nn_amd import _capi
    before = moved(sc)
    sc.set_option(_capi.OPT_INJECT_GIVEUP, _capi.inject_giveup(_capi.INJECT_LOOKBACK, 0, 1))
    got = run_batch(sc, pts, filtered, boxes)
    return got, moved(sc, before)


@pytest.fixture(scope="module")
def setup():
    """the points, the boxes, and per (filtered, boxed) the single-point rounds of a handle that runs nothing else (made once)"""
    import sdpcutsel_via_nn_amd as pkg
    inp = gc.inputs("spar020")
    pts, boxes = batch_points(), batch_boxes(inp["n"])
    single = gc.new_handle(pkg, inp)
    try:
        refs = {(f, b): [run_single(single, pts[p], f, boxes[p] if b else None) for p in range(4)] for f in (False, True) for b in (False, True)}
    finally:
        single.close()
    return pkg, inp, pts, boxes, refs


@pytest.mark.parametrize("boxed", [False, True], ids=["unboxed", "boxed"])
@pytest.mark.parametrize("filtered", [False, True], ids=["plain", "filtered"])
def test_every_verdict_in_one_batch(setup, filtered, boxed):
    from sdpcutsel_via_nn_amd import _capi
    pkg, inp, pts, boxes, refs = setup
    ref, bx = refs[(filtered, boxed)], boxes if boxed else None
    heads = [r["idx"].shape[0] for r in ref]
    # premises of the inputs, on the single-point rounds: the PSD point has nothing violated, a head spans two assembly workgroups
    assert heads[PSD] == 0 and ref[PSD]["rhs"].shape[0] == 0 and max(heads) >= 65 and heads[0] > 0 and heads[3] > 0, heads
    sc = gc.new_handle(pkg, inp)
    try:
        got, d = injected_batch(sc, pts, filtered, bx)
        print("filtered %d boxed %d: heads %s, moved %s" % (filtered, boxed, heads, d))
        for p in range(4):
            assert_same_round(got[p], ref[p], (filtered, boxed, p))
        assert got[PSD]["idx"].shape[0] == 0 and got[PSD]["rhs"].shape[0] == 0 and got[PSD]["values"].shape[0] == 0
        assert d["injected"] == 1
        assert d["redone"] == REDONE_BEFORE
        # one fallback per point with a head (none of them is redone): it went round again; the empty head of the PSD point adds none
        assert d["fallbacks"] == sum(1 for p in range(4) if heads[p] > 0), (d, heads)
        assert sc.box is None and sc.pending is None

        # the same batch undisturbed, and the handle's state behind it
        before = moved(sc)
        again = run_batch(sc, pts, filtered, bx)
        for p in range(4):
            assert_same_round(again[p], ref[p], ("undisturbed", filtered, boxed, p))
        assert moved(sc, before) == {"injected": 0, "fallbacks": 0, "redone": REDONE_BEFORE}
        assert sc.box is None and sc.get_stat(_capi.STAT_SCORED) == 0      # no box, nothing scored: no current point
        with pytest.raises(_capi.SdpCutError):
            sc.round_csr(PLAIN["strat"], PLAIN["sel"])
        sc.set_point(pts[0])
        assert_same_round(sc.round_csr(PLAIN["strat"], PLAIN["sel"], copy=True), refs[(False, False)][0], "round_csr behind the batch")
    finally:
        sc.close()
