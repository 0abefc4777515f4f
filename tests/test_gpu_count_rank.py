"""The sort tail that ranks by counting in one launch (SDPCUT_OPT_COUNT_RANK, csrc/topk_sort.hip: tk_countrank_kernel) against the
tile sort + rank merge it replaces, and against the oracle.

Every case runs the same round on ONE handle with the option off, then on, and requires the two results to be the same bytes:
ids, scores, lambda_min, rhs, coefficient rows, sizes, counters and the strategy switch.  One of the two is then checked against
oracle.rank_arrays on the device's own scores, exactly (the tolerance of the rankings in tests/test_gpu_fuzz.py: index and
ordering work is compared bit for bit).

Lists: 3-variable candidates over 12 variables -- 220 distinct index sets, so a list of 40 000 is ~180 copies of each and nearly
every comparison of the ranking is between EQUAL keys (the tie rules are the common path, not the rare one); 40 000 is above
SDPCUT_PF_MIN_N and the one-workgroup routes, 20 000 is below the fine histogram's limit.  Over 4 variables there are four
distinct index sets: the threshold's tie group is twice the head.
LP points (seeds found on the CPU with the oracle; the regime of the combined strategy is asserted from the device's scores):
  gen     McCormick-feasible, generic: ~200 of the 220 sets violated
  strong  X at the McCormick bound that pays in the objective: ~100 of the 220 sets are strong (positive and violated), more than
          8192 candidates of either list -- the combined strategy resolves STRONG for every head size here
  weak    X at the other bound: ~200 sets violated, none positive -- the combined strategy visits every entry (COMBALL: ties by
          obj_improve, then index) for every head size
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEL_SIZES = [1, 63, 64, 65, 300, 513, 5000, 8192]
# (strategy, point)
REGIMES = {"feas": (1, "gen"), "opt": (2, "gen"), "strong": (4, "strong"), "comball": (4, "weak")}
FIELDS = ("idx", "score", "lam", "rhs", "coef", "ks")


def _point(n, Q_arr, kind):
    rng = np.random.default_rng({"gen": 2, "strong": 1, "weak": 0}[kind])
    iu = np.triu_indices(n)
    x = rng.uniform(0, 1, n)
    lo = np.maximum(0.0, x[iu[0]] + x[iu[1]] - 1.0)
    hi = np.minimum(x[iu[0]], x[iu[1]])
    u = rng.uniform(0, 0.2, lo.shape[0])
    if kind == "gen":
        t = rng.uniform(0, 1, lo.shape[0])
    else:
        t = np.where((Q_arr > 0) == (kind == "weak"), 1 - u, u)
    return np.concatenate([lo + t * (hi - lo), x])


class _List(object):
    """one handle with one candidate list; the device's scores at each point are fetched once and shared"""

    def __init__(self, lib, n, N):
        from sdpcutsel_via_nn_amd import synthetic
        self.n, self.N = n, N
        self.Q, _, _ = synthetic.make_instance(n, 7)
        rng = np.random.default_rng(100 + n)
        self.sets = np.full((N, 5), -1, dtype=np.int32)
        self.sets[:, :3] = synthetic.random_index_sets(n, 3, N, rng)
        self.sc = lib.Scorer(0)
        self.sc.set_builtin_networks(3)
        self.sc.set_instance(n, self.Q)
        self.sc.set_candidates(self.sets, np.full(N, 3, dtype=np.int32))
        self._scores = {}

    def point(self, kind):
        return _point(self.n, self.Q, kind)

    def scores(self, kind):
        from sdpcutsel_via_nn_amd import _capi
        if kind not in self._scores:
            self.sc.set_point(self.point(kind))
            self.sc.score(_capi.EIG | _capi.NN)
            self._scores[kind] = self.sc.get_scores()
        return self._scores[kind]


@pytest.fixture(scope="module")
def lists():
    import sdpcutsel_via_nn_amd as lib
    made = {}

    def get(n, N):
        if (n, N) not in made:
            made[(n, N)] = _List(lib, n, N)
        return made[(n, N)]
    yield get
    for li in made.values():
        li.sc.close()


def _both(li, kind, run):
    """run(scorer) with the option off, then on, each on a fresh point (nothing scored: the round scores for itself)"""
    from sdpcutsel_via_nn_amd import _capi
    out = []
    try:
        for opt in (0, 1):
            li.sc.set_option(_capi.OPT_COUNT_RANK, opt)
            li.sc.set_point(li.point(kind))
            out.append(run(li.sc))
    finally:
        li.sc.set_option(_capi.OPT_COUNT_RANK, 1)
    return out


def _same_round(a, b, what):
    for f in FIELDS:
        assert a[f].shape == b[f].shape and a[f].dtype == b[f].dtype and a[f].tobytes() == b[f].tobytes(), (what, f)
    assert a["n_total"] == b["n_total"] and a["new_strat"] == b["new_strat"] and a["counters"] == b["counters"], what


def _check_oracle(oracle, li, kind, strat, sel, r, regime=None):
    eig, obj = li.scores(kind)
    if regime is not None:
        n_strong = int(((obj > 0) & (eig < -1e-15)).sum())
        assert (n_strong >= min(sel, li.N)) == (regime == "strong"), (regime, n_strong, sel)
    order, ref_score, ref_strat, ref_cnt = oracle.rank_arrays(strat, obj, eig, sel)
    w = min(sel, order.shape[0])
    assert np.array_equal(r["idx"], order[:w]), (kind, strat, sel)
    assert np.array_equal(r["score"], ref_score[:w] + 0.0), (kind, strat, sel)
    assert r["n_total"] == order.shape[0] and r["new_strat"] == ref_strat
    if strat == 4:
        assert r["counters"]["strong"] == ref_cnt["strong"] and r["counters"]["violated"] == ref_cnt["violated"]
    if w:
        assert np.abs(r["lam"] - eig[order[:w]]).max() <= 1e-14


@pytest.mark.parametrize("sel", SEL_SIZES)
@pytest.mark.parametrize("regime", list(REGIMES))
def test_same_round_either_way(lists, oracle, regime, sel):
    strat, kind = REGIMES[regime]
    li = lists(12, 40000)
    a, b = _both(li, kind, lambda sc: sc.select_round(strat, sel))
    _same_round(a, b, (regime, sel))
    _check_oracle(oracle, li, kind, strat, sel, b, regime if strat == 4 else None)


@pytest.mark.parametrize("regime", list(REGIMES))
def test_list_without_the_fine_histogram(lists, oracle, regime):
    strat, kind = REGIMES[regime]
    li = lists(12, 20000)
    a, b = _both(li, kind, lambda sc: sc.select_round(strat, 5000))
    _same_round(a, b, regime)
    _check_oracle(oracle, li, kind, strat, 5000, b, regime if strat == 4 else None)


@pytest.mark.parametrize("strat", [1, 2, 4])
def test_four_distinct_index_sets(lists, oracle, strat):
    """at most four distinct keys in 40 000 candidates: the tie group at the threshold is far larger than the head"""
    li = lists(4, 40000)
    a, b = _both(li, "gen", lambda sc: sc.select_round(strat, 5000))
    _same_round(a, b, strat)
    _check_oracle(oracle, li, "gen", strat, 5000, b)


@pytest.mark.parametrize("regime", ["feas", "comball"])
def test_both_epilogues_agree_on_the_head(lists, regime):
    strat, kind = REGIMES[regime]
    li = lists(12, 40000)
    csr = _both(li, kind, lambda sc: sc.round_csr(strat, 513, copy=True))
    rows = _both(li, kind, lambda sc: {k: (v.copy() if isinstance(v, np.ndarray) else v)
                                       for k, v in sc.select_round(strat, 513, copy=False).items()})
    for f in ("idx", "score", "lam", "ks", "row_entry", "indptr", "indices", "values", "rhs"):
        assert csr[0][f].tobytes() == csr[1][f].tobytes(), f
    _same_round(rows[0], rows[1], regime)
    for f in ("idx", "score", "lam", "ks"):
        assert csr[1][f].tobytes() == rows[1][f].tobytes(), f
    assert csr[1]["new_strat"] == rows[1]["new_strat"] and csr[1]["counters"] == rows[1]["counters"]
    keep = np.flatnonzero(rows[1]["lam"] < -1e-15)
    assert np.array_equal(csr[1]["row_entry"], keep) and np.array_equal(csr[1]["rhs"], rows[1]["rhs"][keep])


@pytest.mark.parametrize("regime", ["feas", "opt", "comball"])
def test_big_heads_keep_the_two_kernels(lists, oracle, regime):
    """a head of 9000 entries is beyond the one-launch path (and beyond the device-resolved regime of the combined strategy,
    which the library serves by its general path): the tile sort and the keys-only merge answer with the option on or off"""
    strat, kind = REGIMES[regime]
    li = lists(12, 40000)
    a, b = _both(li, kind, lambda sc: sc.select_round(strat, 9000))
    _same_round(a, b, regime)
    _check_oracle(oracle, li, kind, strat, 9000, b)


@pytest.mark.parametrize("strat", [1, 2])
def test_sharded_round_at_world_size_one(oracle, strat):
    """the shard record (header and padding behind the head) is written by the rank merge: the sharded round keeps the two
    kernels whatever the option says"""
    import torch
    import sdpcutsel_via_nn_amd as lib
    from sdpcutsel_via_nn_amd import _capi
    from sdpcutsel_via_nn_amd.distributed import DeviceOps, ShardedSelector
    li = _List(lib, 12, 40000)
    try:
        eig, obj = li.scores("gen")
        sel = ShardedSelector(DeviceOps(li.sc, torch.device("cuda", 0)), li.N)
        out = []
        for opt in (0, 1):
            li.sc.set_option(_capi.OPT_COUNT_RANK, opt)
            li.sc.set_point(li.point("gen"))
            out.append(sel.select_round(strat, 300))
        a, b = out
        for f in ("ids", "scores", "mine", "lam", "coef", "rhs", "ks"):
            assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), f
        assert a["new_strat"] == b["new_strat"] and a["n_total"] == b["n_total"] and a["counters"] == b["counters"]
        order, ref_score, _, _ = oracle.rank_arrays(strat, obj, eig, 300)
        assert np.array_equal(b["ids"], order[:300]) and np.array_equal(b["scores"], ref_score[:300] + 0.0)
        assert sel.path_counts["common"] == 2 and b["mine"].all()
    finally:
        li.sc.set_stream(None)
        li.sc.close()
