"""The give-up paths of the two families of bounded device waits -- the fused top-k selection (csrc/topk_passes.hip) and the
look-back of the ordered CSR row assembly (csrc/rows_dev.h) -- made to run by SDPCUT_OPT_INJECT_GIVEUP (include/sdpcut.h) and held
against undisturbed handles, byte for byte.  The table, its inputs and the runner are tests/giveup_cases.py; DESIGN.md section 5
"Give-up paths" has the accounting of SDPCUT_STAT_SELECT_FALLBACKS the cases assert.  Run with -s for one line per case:
injections, fallbacks and the case's other statistic."""
import numpy as np
import pytest

import giveup_cases as gc
from sdpcutsel_via_nn_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import sdpcutsel_via_nn_amd as pkg
    return pkg


def _say(line):
    print("\n[giveup] " + line, end="")


@pytest.mark.parametrize("cid", [c["id"] for c in gc.CASES])
def test_giveup_case(lib, cid):
    gc.run_case(lib, gc.BY_ID[cid], report=_say)


def test_option_contract(lib):
    """0 is the default and disarms; the option disarms itself when consumed; launches without a bounded wait consume nothing;
    refused with SDPCUT_ESTATE while a round is pending; values outside the encoding are refused"""
    inp = gc.inputs("generic")
    sc = gc.new_handle(lib, inp)
    try:
        ref = gc.call_round_csr(sc, inp, 1, 300)
        assert sc.get_stat(_capi.STAT_INJECTED) == 0 and sc.get_stat(_capi.STAT_SELECT_FALLBACKS) == 0
        # armed and disarmed by hand: nothing happens
        sc.set_option(_capi.OPT_INJECT_GIVEUP, _capi.inject_giveup(gc.SELECT))
        sc.set_option(_capi.OPT_INJECT_GIVEUP, 0)
        gc.same(ref, gc.call_round_csr(sc, inp, 1, 300), "disarmed by hand")
        assert sc.get_stat(_capi.STAT_INJECTED) == 0 and sc.get_stat(_capi.STAT_SELECT_FALLBACKS) == 0
        # first = 1, count = 1: the first round passes, the second is hit, the third passes again
        sc.set_option(_capi.OPT_INJECT_GIVEUP, _capi.inject_giveup(gc.SELECT, 1, 1))
        for want_inj, want_fb in ((0, 0), (1, 1), (1, 1)):
            gc.same(ref, gc.call_round_csr(sc, inp, 1, 300), "first = 1")
            assert (sc.get_stat(_capi.STAT_INJECTED), sc.get_stat(_capi.STAT_SELECT_FALLBACKS)) == (want_inj, want_fb)
        # a head of 64 entries is one workgroup: no look-back, not a launch of the site -- the arming waits for the next longer head
        sc.set_option(_capi.OPT_INJECT_GIVEUP, _capi.inject_giveup(gc.LOOKBACK))
        gc.call_round_csr(sc, inp, 1, 64)
        assert (sc.get_stat(_capi.STAT_INJECTED), sc.get_stat(_capi.STAT_SELECT_FALLBACKS)) == (1, 1)
        gc.same(ref, gc.call_round_csr(sc, inp, 1, 300), "after a short head")
        assert (sc.get_stat(_capi.STAT_INJECTED), sc.get_stat(_capi.STAT_SELECT_FALLBACKS)) == (2, 2)
        # refused while a round is pending, whatever the value; the pending round is untouched
        sc.round_csr_begin(1, 300, point=inp["points"]["gen"])
        for v in (0, _capi.inject_giveup(gc.SELECT)):
            with pytest.raises(_capi.SdpCutError, match="pending"):
                sc.set_option(_capi.OPT_INJECT_GIVEUP, v)
        gc.same(ref, gc._copy(sc.round_csr_end(copy=True)), "pending round")
        for bad in (-1, 1, (3 << 16) | 1, 1 << 16, (1 << 16) | (1 << 8), 1 << 24):
            with pytest.raises(ValueError, match="SDPCUT_OPT_INJECT_GIVEUP"):
                sc.set_option(_capi.OPT_INJECT_GIVEUP, bad)
        assert (sc.get_stat(_capi.STAT_INJECTED), sc.get_stat(_capi.STAT_SELECT_FALLBACKS)) == (2, 2)
    finally:
        sc.close()


def test_one_workgroup_selections_are_no_site(lib):
    """the mixed cover (142 sets) and the spar020 cover (1051) are selected by one workgroup, the batched points by tk_points_kernel:
    an armed selection site is not consumed by them"""
    for name in ("mixed", "spar020"):
        inp = gc.inputs(name)
        sc = gc.new_handle(lib, inp)
        try:
            ref = gc.call_round_csr(sc, inp, 4, 129)
            sc.set_option(_capi.OPT_INJECT_GIVEUP, _capi.inject_giveup(gc.SELECT))
            gc.same(ref, gc.call_round_csr(sc, inp, 4, 129), name)
            if name == "spar020":
                gc.call_points(sc, inp, 1, 129)
            assert sc.get_stat(_capi.STAT_INJECTED) == 0 and sc.get_stat(_capi.STAT_SELECT_FALLBACKS) == 0
            sc.set_option(_capi.OPT_INJECT_GIVEUP, 0)
        finally:
            sc.close()


# ---- S6: the sharded round -------------------------------------------------------------------------------------------------------------
def _round_fields(r):
    return {f: np.asarray(r[f]).copy() for f in ("ids", "scores", "mine", "lam", "coef", "rhs", "ks")}


@pytest.mark.parametrize("strat", [1, 2])
def test_sharded_round_world_one_void_head(lib, strat):
    """S6: ShardedSelector.select_round whose shard head is void answers through the unfused route: the same ids, scores and rows"""
    import torch
    from sdpcutsel_via_nn_amd.distributed import DeviceOps, ShardedSelector
    inp = gc.inputs("generic")
    dev = torch.device("cuda", 0)
    a, b = gc.new_handle(lib, inp), gc.new_handle(lib, inp)
    try:
        sa, sb = ShardedSelector(DeviceOps(a, dev), a.N), ShardedSelector(DeviceOps(b, dev), b.N)
        a.set_point(inp["points"]["gen"])
        ra = sa.select_round(strat, 300)
        assert sa.path_counts["common"] == 1 and sa.path_counts["unfused"] == 0
        b.set_point(inp["points"]["gen"])
        b.set_option(_capi.OPT_INJECT_GIVEUP, _capi.inject_giveup(gc.SELECT))
        rb = sb.select_round(strat, 300)
        _say("S6-world1-s%d  injected %d  fallbacks %d  unfused %d" % (strat, b.get_stat(_capi.STAT_INJECTED),
                                                                     b.get_stat(_capi.STAT_SELECT_FALLBACKS), sb.path_counts["unfused"]))
        assert b.get_stat(_capi.STAT_INJECTED) == 1
        assert sb.path_counts["unfused"] == 1 and sb.path_counts["common"] == 0
        # (the sharded calls have no host wait of their own to count a fallback at: the record's word 4 is the report)
        assert b.get_stat(_capi.STAT_SELECT_FALLBACKS) == 0
        fa, fb = _round_fields(ra), _round_fields(rb)
        for f in ("ids", "scores", "mine", "lam", "rhs", "ks"):
            assert fa[f].tobytes() == fb[f].tobytes(), f
        w = b.row_len
        assert fa["coef"][:, :w].tobytes() == np.ascontiguousarray(fb["coef"][:, :w]).tobytes()
        assert ra["new_strat"] == rb["new_strat"] and ra["n_total"] == rb["n_total"]
        # the next sharded round on the same handle is the common one again
        b.set_point(inp["points"]["new"])
        a.set_point(inp["points"]["new"])
        fa, fb = _round_fields(sa.select_round(strat, 300)), _round_fields(sb.select_round(strat, 300))
        for f in fa:
            assert fa[f].tobytes() == fb[f].tobytes(), f
        assert sb.path_counts["common"] == 1 and b.get_stat(_capi.STAT_INJECTED) == 1
        for sc in (a, b):
            sc.set_stream(None)
        gc.same(gc.followup_reference(lib, inp, None), gc.followup(b, inp), "S6 follow-up")
    finally:
        a.set_stream(None)
        b.set_stream(None)
        a.close()
        b.close()


def test_sharded_round_ragged_shard_zero_void(lib):
    """S6: the four-handle form of test_shard_round_ragged_shards_one_process with shard 0's head void: word 4 of the merged
    headers is non-zero on every rank, and what ShardedSelector.end_round does next -- every shard ranks for itself, the heads
    are merged, each shard makes its own rows -- gives the undisturbed merged head"""
    import torch
    from sdpcutsel_via_nn_amd import networks, synthetic
    from sdpcutsel_via_nn_amd.distributed import DeviceOps
    dev = torch.device("cuda", 0)
    sizes = [20000, 0, 7, 12000]
    bases = np.concatenate([[0], np.cumsum(sizes)])
    nv, sel, strat = 40, 300, 1
    wl = synthetic.make_workload(nb_vars=nv, k=3, count=int(bases[-1]), seed=23)
    opss = []
    try:
        for r, n in enumerate(sizes):
            sc = _capi.Scorer(0)
            sc.set_network(3, *networks.load_network(3))
            sc.set_instance(nv, wl["Q_arr"])
            lo = int(bases[r])
            sc.set_candidates(wl["set_inds"][lo:lo + n], wl["ks"][lo:lo + n], global_base=lo)
            opss.append(DeviceOps(sc, dev))

        def sharded_round():
            for ops in opss:
                ops.scorer.set_point(wl["vars_values"])
            allrec = torch.cat([ops.shard_head(strat, sel) for ops in opss])
            return [{k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in ops.shard_finish(len(sizes), sel, allrec, sel).items()}
                    for ops in opss]

        good = sharded_round()
        assert all(int(o["headers"].sum(axis=0)[4]) == 0 for o in good)
        opss[0].scorer.set_option(_capi.OPT_INJECT_GIVEUP, _capi.inject_giveup(gc.SELECT))
        void = sharded_round()
        assert [ops.scorer.get_stat(_capi.STAT_INJECTED) for ops in opss] == [1, 0, 0, 0]
        for o in void:
            assert int(o["headers"][0][4]) != 0 and int(o["headers"].sum(axis=0)[4]) != 0
            assert all(int(o["headers"][r][4]) == 0 for r in (1, 2, 3))
        # the unfused route, one process standing in for four ranks
        heads_i, heads_s = [], []
        for ops in opss:
            if ops.scorer.N:
                ops.ensure_scored(strat)
                idx, score, _, _, _ = ops.scorer.rank(strat, sel, max_out=sel)
                heads_i.append(idx)
                heads_s.append(score)
        ids, scores = np.concatenate(heads_i), np.concatenate(heads_s)
        order = np.lexsort((ids, -scores))[:sel]
        ids, scores = ids[order], scores[order]
        k = min(sel, int(good[0]["headers"].sum(axis=0)[0]))
        assert np.array_equal(ids[:k], good[0]["idx"][:k]) and scores[:k].tobytes() == good[0]["score"][:k].tobytes()
        for r, ops in enumerate(opss):
            mine, lam, coef, rhs, ks = ops.rows_of(ids[:k])
            own = good[r]["ks"][:k] > 0
            assert np.array_equal(mine, own)
            assert lam.tobytes() == good[r]["lam"][:k][own].tobytes() and rhs.tobytes() == good[r]["rhs"][:k][own].tobytes()
            assert np.array_equal(ks, good[r]["ks"][:k][own])
        # and the next sharded round is whole again
        again = sharded_round()
        for o, g in zip(again, good):
            for f in ("headers", "idx", "score", "lam", "rhs", "ks"):
                assert np.asarray(o[f]).tobytes() == np.asarray(g[f]).tobytes(), f
        _say("S6-ragged-shard0  injected %s  fallbacks %s" % ([ops.scorer.get_stat(_capi.STAT_INJECTED) for ops in opss],
                                                               [ops.scorer.get_stat(_capi.STAT_SELECT_FALLBACKS) for ops in opss]))
    finally:
        for ops in opss:
            ops.scorer.set_stream(None)
            ops.scorer.close()
