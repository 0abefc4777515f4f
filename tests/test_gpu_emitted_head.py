"""The head of a combined round selected from the list its scoring launch emitted (csrc/topk_route.h: TK_ROUTE_EMITTED; the
skipping kernels of csrc/score_mfma.hip append every strong candidate's (key, index), tk_refine_kernel<true, true> compacts the
head's superset from that list in the strong regime), against the same round on a fresh handle with SDPCUT_OPT_EMIT_HEAD = 0, which
takes TK_ROUTE_ONFLY: every field of the round equal byte for byte.

Two lists under SDPCUT_OPT_SKIP_NONVIOLATED = 2, both long enough for the score launch to count for the selection (more than 12 288
candidates: shorter lists are selected by one workgroup and never reach either route):
  short  12 500 candidates, below SDPCUT_PF_MIN_N: no fine histogram, the strong class fits the sort buffers and is taken whole;
  long   40 000 candidates: the threshold comes from the fine histogram.
Each holds exactly S = 600 strong candidates -- copies of the 52 strong sets of the pattern list, so every key occurs about a dozen
times and a head shorter than S cuts through a group of equal keys.  Heads: S - 100 and S // 2 (strong count above sel, equal keys
across the threshold), S (equal to sel), S + 1 (one below sel: the other regime, the list must not be read).  Then a capacity forced
below S (the overflow flag, the scan of the scores instead) and several rounds on one handle (the count and the flag are the
round's own).  A third list holds 9 000 strong candidates, more than the sort buffers' 8192: it is served from the list only through
the threshold of the fine histogram, so with SDPCUT_OPT_PREFILTER = 0, or with a head of 8192 whose superset cannot fit, every
workgroup must still be there to scan the scores.  SDPCUT_STAT_EMITTED_SELECTIONS says which way a selection went; SDPCUT_STAT_SELECT_FALLBACKS must stay 0 throughout."""
import numpy as np
import pytest

import test_gpu_skip_nonviolated as base

pytestmark = pytest.mark.gpu

S = 600
S_BIG = 9000
SIZES = {"short": 12500, "long": 40000}
CSR_FIELDS, FIELDS = base.CSR_FIELDS, base.FIELDS


@pytest.fixture(scope="module")
def world(oracle):
    return base._World(oracle)


def _list(world, n, seed, S=S):
    """-> index into ALL_SETS of n candidates: about half violated, exactly S of them strong at point 3"""
    rng = np.random.default_rng(seed)
    viol_pool = np.setdiff1d(np.flatnonzero(~base.NONVIOL), world.strong)
    free_pool = np.flatnonzero(base.NONVIOL)
    flags = rng.uniform(size=n) < 0.5
    which = np.where(flags, rng.choice(viol_pool, size=n), rng.choice(free_pool, size=n))
    spots = rng.choice(np.flatnonzero(flags), size=S, replace=False)
    which[spots] = world.strong[rng.integers(world.strong.size, size=S)]
    assert int(np.isin(which, world.strong).sum()) == S
    return which


def _handle(world, which, emit_head=1, emit_cap=0):
    import sdpcutsel_via_nn_amd as lib
    from sdpcutsel_via_nn_amd import _capi
    sets = np.full((which.shape[0], 5), -1, dtype=np.int32)
    sets[:, :3] = base.ALL_SETS[which]
    sc = lib.Scorer(0)
    sc.set_builtin_networks(5)
    sc.set_instance(base.N_VARS, world.Q)
    sc.set_candidates(sets, np.full(which.shape[0], 3, dtype=np.int32))
    sc.set_option(_capi.OPT_SKIP_NONVIOLATED, 2)
    sc.set_option(_capi.OPT_EMIT_HEAD, emit_head)
    sc.set_option(_capi.OPT_EMIT_CAP, emit_cap)
    return sc


def _round(sc, call, sel, vv):
    """one combined round at a fresh point -> (the round, selections from the emitted list it added, fallbacks it added)"""
    from sdpcutsel_via_nn_amd import _capi
    e0, f0 = sc.get_stat(_capi.STAT_EMITTED_SELECTIONS), sc.get_stat(_capi.STAT_SELECT_FALLBACKS)
    sc.set_point(vv)
    out = getattr(sc, call)(4, sel, copy=True)
    return out, sc.get_stat(_capi.STAT_EMITTED_SELECTIONS) - e0, sc.get_stat(_capi.STAT_SELECT_FALLBACKS) - f0


@pytest.fixture(scope="module")
def handles(world):
    made = {}

    def get(size):
        if size not in made:
            which = _list(world, SIZES[size], seed=11 + SIZES[size])
            made[size] = (_handle(world, which), _handle(world, which, emit_head=0), which)
        return made[size]
    yield get
    for new, old, _ in made.values():
        new.close()
        old.close()


@pytest.mark.parametrize("size", sorted(SIZES))
def test_same_round_from_the_emitted_list(world, handles, size):
    new, old, which = handles(size)
    vv = world.points[3]
    for sel in (S - 100, S // 2, S, S + 1):
        for call, fields in (("round_csr", CSR_FIELDS), ("select_round", FIELDS)):
            a, ea, fa = _round(new, call, sel, vv)
            b, eb, fb = _round(old, call, sel, vv)
            print(size, sel, call, "emitted selections", ea, eb, "fallbacks", fa, fb, "counters", a["counters"], "new_strat", a["new_strat"])
            base._same(a, b, fields, (size, sel, call))
            assert a["idx"].shape[0] == sel
            assert fa == 0 and fb == 0 and eb == 0
            # the strong regime (at least sel strong candidates) reads the list; one strong candidate short of sel it must not
            assert ea == (1 if sel <= S else 0), (size, sel, call, ea)
            if sel <= S:
                assert np.isin(which[a["idx"]], world.strong).all()


@pytest.mark.parametrize("size", sorted(SIZES))
def test_overflow_scans_the_scores(world, handles, size):
    from sdpcutsel_via_nn_amd import _capi
    _, old, which = handles(size)
    vv = world.points[3]
    small = _handle(world, which, emit_cap=S - 37)
    try:
        for sel in (S - 100, S):
            a, ea, fa = _round(small, "round_csr", sel, vv)
            b, _, fb = _round(old, "round_csr", sel, vv)
            base._same(a, b, CSR_FIELDS, (size, sel, "overflow"))
            assert ea == 0 and fa == 0 and fb == 0, (size, sel, ea, fa, fb)
        # the same handle with the capacity back: the flag and the count of the rounds before are gone
        small.set_option(_capi.OPT_EMIT_CAP, 0)
        for sel in (S, S - 100, S):
            a, ea, fa = _round(small, "round_csr", sel, vv)
            b, _, _ = _round(old, "round_csr", sel, vv)
            base._same(a, b, CSR_FIELDS, (size, sel, "after the overflow"))
            assert ea == 1 and fa == 0, (size, sel, ea, fa)
        # ... and an overflow behind rounds that read the list
        small.set_option(_capi.OPT_EMIT_CAP, 1)
        a, ea, fa = _round(small, "round_csr", S, vv)
        b, _, _ = _round(old, "round_csr", S, vv)
        base._same(a, b, CSR_FIELDS, (size, "capacity 1"))
        assert ea == 0 and fa == 0
    finally:
        small.close()


def test_two_points_on_one_handle(world, handles):
    """rounds at alternating LP points on one handle: the strong class of point 0 is another one, every round reads its own list"""
    new, old, _ = handles("long")
    for s, sel in ((3, S), (0, 40), (3, S - 100), (0, 40)):
        a, ea, fa = _round(new, "round_csr", sel, world.points[s])
        b, _, _ = _round(old, "round_csr", sel, world.points[s])
        base._same(a, b, CSR_FIELDS, (s, sel))
        print("point", s, "sel", sel, "emitted selections", ea, "counters", a["counters"], "new_strat", a["new_strat"])
        assert fa == 0
        if s == 3:
            assert ea == 1


def test_a_class_beyond_the_sort_buffers(world):
    from sdpcutsel_via_nn_amd import _capi
    which = _list(world, 40000, seed=5, S=S_BIG)
    new, old = _handle(world, which), _handle(world, which, emit_head=0)
    vv = world.points[3]
    try:
        for prefilter in (1, 0, 1):
            for sc in (new, old):
                sc.set_option(_capi.OPT_PREFILTER, prefilter)
            for sel in (5000, 8192, 300):
                d0 = new.get_stat(_capi.STAT_DIRECT_SELECTIONS)
                a, ea, fa = _round(new, "round_csr", sel, vv)
                direct = new.get_stat(_capi.STAT_DIRECT_SELECTIONS) - d0
                b, eb, fb = _round(old, "round_csr", sel, vv)
                print("prefilter", prefilter, "sel", sel, "emitted selections", ea, "direct", direct, "fallbacks", fa, fb, a["counters"])
                base._same(a, b, CSR_FIELDS, (prefilter, sel))
                assert a["idx"].shape[0] == sel and fa == 0 and fb == 0 and eb == 0
                # 9 000 members do not fit the sort buffers: the list serves exactly when the fine histogram gave the threshold
                assert ea == direct, (prefilter, sel, ea, direct)
                if not prefilter:
                    assert ea == 0
    finally:
        new.close()
        old.close()
