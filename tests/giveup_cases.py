"""The give-up paths of the bounded device waits, reached by injection (SDPCUT_OPT_INJECT_GIVEUP, include/sdpcut.h): the case table
of tests/test_gpu_giveup.py, its inputs, and the runner every case goes through.  A plain module: no fixtures; nothing here touches
the GPU until `run_case` is called.  tests/test_giveup_cpu.py checks the table against CONSUMERS without a device.

Shape of a case (run_case).  Handle A runs the call undisturbed; handle B, set up identically, arms the injection and runs the same
call.  Then: every array and scalar B returns equals A's byte for byte (cases with `against` compare with a handle in another
setup: the exact-head round that gave up is the option-off round); SDPCUT_STAT_INJECTED rose by `injected`;
SDPCUT_STAT_SELECT_FALLBACKS by `fallbacks` and the statistics of `stats` by their amounts (taken from the host code, DESIGN.md
section 5 "Give-up paths"; never from a run); the follow-up -- a fused select_round under another strategy at a new point, a
round_csr with a head of 65 or more, score + rank -- returns on B what it returns on a fresh handle, and moves neither of the two
statistics.  An error leg (`error`) raises SdpCutError with the library's message, leaves no round pending, and the follow-up holds
on the same handle.

Sites and what consumes their marks: CONSUMERS names every host path the two marks reach; a case lists the ones it runs through.

Inputs.  generic: n = 30, k = 3, N = 20 000 (synthetic.make_workload) -- longer than the sort buffers and the one-workgroup routes, so
every selection is a launch of the site; its selection stops early or resolves directly, no workgroup waits.  nopf: the same with
SDPCUT_OPT_PREFILTER = 0 (the radix passes).  tie: the four distinct index sets of test_gpu_count_rank.py (n = 4, N = 40 000):
masses of equal keys, the selection runs its later digits behind the published states and the grid barrier -- the input on which
workgroups leave AT a wait (premise: no direct selection served it, SDPCUT_STAT_DIRECT_SELECTIONS stays 0 on the undisturbed
handle).  mixed: the dim-5 cover of spar040-030-1 (142 sets, k = 2 .. 5), heads of 65, 129 and the whole list.  skip: all-ones
adjacency n = 40, N = 70 000 triples drawn with repeats (> 65 536: SDPCUT_OPT_SKIP_NONVIOLATED = 1 skips) at a point with more than
half of the list strong.  vertex: the structured vertex of test_gpu_round4.py (x = 0.5, X = 0.1; the candidates without a positive
measure plus sixty with one), whose every-entry-visited round goes through topk_tie_split.  spar020: the dim-3 cover of
spar020-100-1 (1051 sets) with the eight blended points of diverse_points_cases.py."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from sdpcutsel_via_nn_amd import _capi      # noqa: E402

SELECT, LOOKBACK = _capi.INJECT_SELECT, _capi.INJECT_LOOKBACK
GOLDEN = os.path.join(HERE, "golden")

# every host path that consumes one of the two marks: key -> (file, what happens there)
CONSUMERS = {
    "round.skipped_void": ("csrc/round.hip", "round_end: a skipped / filtered combined round whose selection is void completes the measure and begins again"),
    "round.exact_gives_up": ("csrc/round.hip", "round_end: an exact head whose band selection is void gives up to the ordinary round"),
    "round.csr_head_again": ("csrc/round.hip", "round_end: the enqueued assembly gave up, csr_head_again(.., 1)"),
    "round.general_path": ("csrc/round.hip", "round_end: void selection -> rank_on_device and emit_head"),
    "round.csr_assemble_wait": ("csrc/round.hip", "csr_assemble_wait and its count_failure rule"),
    "rank.fast_finish": ("csrc/rank.hip", "rank_fast_finish: c4[4] -> 0"),
    "rank.on_device": ("csrc/rank.hip", "rank_on_device: a void fast attempt, a void every-entry-visited selection -> the full sorts"),
    "topk.tie_split_void": ("csrc/topk.hip", "topk_tie_split: one of its own selections is void -> 1, the general path answers"),
    "tri.relaunch": ("csrc/tri.hip", "tri_separate: once more with fused_tail off, then 'selection void'"),
    "points.again": ("csrc/points.hip", "round_points serving round_csr_points[_boxed]: the `again` list and 'timed out twice'"),
    "points.diverse_again": ("csrc/points.hip", "round_points serving round_csr_points_diverse: the same `again` list, 'timed out twice' under its name"),
    "shard.void_record": ("csrc/shard.hip", "a void head writes nothing behind the record's header, word 4 set"),
    "distributed.unfused": ("sdpcutsel_via_nn_amd/distributed.py", "ShardedSelector.end_round: a void record -> the unfused route"),
}

FB = _capi.STAT_SELECT_FALLBACKS
STAT_NAMES = {"nn_completions": _capi.STAT_NN_COMPLETIONS, "exact_gave_up": _capi.STAT_EXACT_GAVE_UP, "tie_splits": _capi.STAT_TIE_SPLITS,
              "points_redone": _capi.STAT_POINTS_REDONE, "rounds": _capi.STAT_ROUNDS}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _gen_point(n, Q_arr, kind):
    """the points of test_gpu_count_rank.py: gen (random in the McCormick interval), strong / weak (X pushed by the sign of Q)"""
    rng = np.random.default_rng({"gen": 2, "strong": 1, "weak": 0, "new": 5}[kind])
    iu = np.triu_indices(n)
    x = rng.uniform(0.3, 0.7, n) if kind == "strong" else rng.uniform(0, 1, n)
    lo = np.maximum(0.0, x[iu[0]] + x[iu[1]] - 1.0)
    hi = np.minimum(x[iu[0]], x[iu[1]])
    u = rng.uniform(0, 0.2, lo.shape[0])
    t = rng.uniform(0, 1, lo.shape[0]) if kind in ("gen", "new") else np.where((Q_arr > 0) == (kind == "weak"), 1 - u, u)
    return np.concatenate([lo + t * (hi - lo), x])


def _pad(sets):
    out = np.full((sets.shape[0], 5), -1, dtype=np.int32)
    out[:, :sets.shape[1]] = sets
    return out


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict(n, Q, sets [N, 5], ks [N], points {kind: vv}, options {id: value}, lpobj or None)"""
    from sdpcutsel_via_nn_amd import harness, synthetic
    opts, lpobj = {}, None
    if name in ("n20", "n40"):      # the lists of the triangle cases: the follow-up needs one, on the instance size of the graph
        n = int(name[1:])
        Q, _, _ = synthetic.make_instance(n, 7)
        sets = _pad(synthetic.random_index_sets(n, 3, 20000, np.random.default_rng(100 + n)))
        ks = np.full(20000, 3, dtype=np.int32)
    elif name in ("generic", "nopf", "exact", "exact_off", "nofuse"):
        wl = synthetic.make_workload(nb_vars=30, k=3, count=20000, seed=7)
        n, Q, sets, ks = 30, wl["Q_arr"], wl["set_inds"], wl["ks"]
        if name == "nopf":
            opts[_capi.OPT_PREFILTER] = 0
        if name == "exact":
            opts[_capi.OPT_EXACT_HEAD] = 1
        if name == "nofuse":      # the combined regime resolved by the host: a weak point's round goes through rank_on_device + emit_head
            opts[_capi.OPT_FUSE_KEYS] = 0
            opts[_capi.OPT_AUTO_REGIME] = 0
    elif name == "tie":
        n = 4
        Q, _, _ = synthetic.make_instance(n, 7)
        sets = _pad(synthetic.random_index_sets(n, 3, 40000, np.random.default_rng(100 + n)))
        ks = np.full(40000, 3, dtype=np.int32)
    elif name == "skip":
        n = 40
        Q, _, _ = synthetic.make_instance(n, 7)
        sets = _pad(synthetic.random_index_sets(n, 3, 70000, np.random.default_rng(204)))
        ks = np.full(70000, 3, dtype=np.int32)
        opts[_capi.OPT_SKIP_NONVIOLATED] = 1
        opts[_capi.OPT_FP32_FILTER] = 1
    elif name in ("mixed", "spar020"):
        fname, dim = {"mixed": ("spar040-030-1.in", 5), "spar020": ("spar020-100-1.in", 3)}[name]
        inst = harness.parse_boxqp(os.path.join(GOLDEN, "instances", fname))
        S, k_arr, _ = _capi.enumerate_cover(inst["adj"], dim)
        n, Q = inst["nb_vars"], np.asarray(inst["Q_arr"], dtype=np.float64)
        sets, ks = np.ascontiguousarray(S, dtype=np.int32), np.ascontiguousarray(k_arr, dtype=np.int32)
        lpobj = np.concatenate([Q, np.asarray(inst["c"], dtype=np.float64)])
    elif name == "vertex":
        raise KeyError("the vertex list needs the device's scores: vertex_inputs(lib)")
    else:
        raise KeyError(name)
    if lpobj is None:
        rng = np.random.default_rng(31)
        lpobj = np.concatenate([Q, rng.uniform(-1, 1, n)])
    pts = {kind: _gen_point(n, Q, kind) for kind in ("gen", "strong", "weak", "new")}
    if name in ("mixed", "spar020"):
        pts["gen"] = harness.random_mccormick_point(n, np.random.default_rng(700))
    return dict(name=name, n=n, Q=Q, sets=sets, ks=ks, points=pts, options=opts, lpobj=lpobj)


_VERTEX = {}


def vertex_inputs(lib):
    """the structured vertex of test_gpu_round4.py at 120 000 drawn triples: the list is chosen by the device's own scores (made once)"""
    if "v" not in _VERTEX:
        from sdpcutsel_via_nn_amd import synthetic
        n = 100
        wl = synthetic.make_workload(nb_vars=n, k=3, count=120000, seed=7)
        vv = np.concatenate([np.full((n, n), 0.1)[np.triu_indices(n)], np.full(n, 0.5)])
        sc = lib.Scorer(0)
        try:
            sc.set_builtin_networks(3)
            sc.set_instance(n, wl["Q_arr"])
            sc.set_candidates(wl["set_inds"], wl["ks"])
            sc.set_point(vv)
            sc.score(_capi.EIG | _capi.NN)
            _, obj0 = sc.get_scores()
        finally:
            sc.close()
        keep = np.sort(np.concatenate([np.flatnonzero(obj0 <= 0), np.flatnonzero(obj0 > 0)[:60]]))
        assert keep.size > 12288, keep.size      # beyond the one-workgroup routes: the round's own selection is a launch of the site
        rng = np.random.default_rng(31)
        pts = {kind: _gen_point(n, wl["Q_arr"], kind) for kind in ("strong", "weak", "new")}
        pts["gen"] = vv
        _VERTEX["v"] = dict(name="vertex", n=n, Q=wl["Q_arr"], sets=wl["set_inds"][keep], ks=wl["ks"][keep], points=pts, options={},
                            lpobj=np.concatenate([wl["Q_arr"], rng.uniform(-1, 1, n)]))
    return _VERTEX["v"]


def get_inputs(lib, name):
    return vertex_inputs(lib) if name == "vertex" else inputs(name)


@functools.lru_cache(maxsize=None)
def tri_inputs(name):
    """-> (n, adjacency, LP point) of the triangle cases: the n = 20 golden instance and a random graph on 40 vertices"""
    from sdpcutsel_via_nn_amd import harness
    if name == "golden20":
        g = np.load(os.path.join(GOLDEN, "inst_tri.npz"))
        return int(g["spar020_100_1_nb_vars"]), g["spar020_100_1_adj"], g["spar020_100_1_rnd_0p5_vars"]
    n = 40
    rng = np.random.default_rng(5)
    adj = np.triu(rng.uniform(size=(n, n)) < 0.75, 1)
    adj = adj | adj.T
    return n, adj, harness.random_mccormick_point(n, np.random.default_rng(41))


def new_handle(lib, inp, tri=None):
    """a handle with the networks, the options and the instance of `inp`, its list, its objective; tri: (n, adj, vv) adds the table"""
    sc = lib.Scorer(0)
    try:
        sc.set_builtin_networks(5)
        for opt in sorted(inp["options"]):
            sc.set_option(opt, inp["options"][opt])
        sc.set_instance(inp["n"], inp["Q"])
        sc.set_candidates(inp["sets"], inp["ks"])
        sc.set_objective(inp["lpobj"])
        sc.set_efficacy_weight(0.1)
        if tri is not None:
            sc.tri_preprocess(tri[1])
    except Exception:
        sc.close()
        raise
    return sc


# ---- the calls --------------------------------------------------------------------------------------------------------------------------
def _copy(r):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}


def _list(rs):
    out = {}
    for p, r in enumerate(rs):
        for k, v in _copy(r).items():
            out["p%d.%s" % (p, k)] = v
    return out


def call_select_round(sc, inp, strat, sel, point="gen"):
    sc.set_point(inp["points"][point])
    return _copy(sc.select_round(strat, sel))


def call_round_csr(sc, inp, strat, sel, point="gen"):
    return _copy(sc.round_csr(strat, sel, point=inp["points"][point], copy=True))


def call_begin_end(sc, inp, strat, sel, point="gen"):
    sc.round_csr_begin(strat, sel, point=inp["points"][point])
    return _copy(sc.round_csr_end(copy=True))


def call_rank(sc, inp, strat, sel, point="gen"):
    sc.set_point(inp["points"][point])
    sc.score({1: _capi.EIG, 2: _capi.NN, 4: _capi.EIG | _capi.NN, 6: _capi.EIG | _capi.EFF}[strat])
    idx, score, n_total, new_strat, cnt = sc.rank(strat, sel, max_out=sel)
    return dict(idx=idx, score=score, n_total=n_total, new_strat=new_strat, counters=cnt)


def call_skipped_round(sc, inp, strat, sel, point="strong"):
    return _copy(sc.round_csr(strat, sel, point=inp["points"][point], copy=True))


def call_diverse(sc, inp, strat, sel, point="gen"):
    return _copy(sc.round_csr_diverse(inp["points"][point], strat, sel, 0.5, pool_size=4 * sel, copy=True))


def call_multi(sc, inp, strat, sel, quota, point="gen"):
    return _copy(sc.round_csr_multi(inp["points"][point], strat, sel, 5, row_quota=quota, copy=True))


def _batch(inp, boxed):
    import diverse_points_cases as dc
    assert inp["name"] == "spar020"
    if boxed:
        return dc.boxes_and_points("spar020", 8)
    return None, dc.points("spar020")


def call_points(sc, inp, strat, sel, boxed=False):
    boxes, pts = _batch(inp, boxed)
    return _list(sc.round_csr_points(pts, strat, sel, copy=True, boxes=boxes))


def call_points_diverse(sc, inp, strat, sel, pool, boxed=False):
    boxes, pts = _batch(inp, boxed)
    # (max_parallel = 1: the walk accepts every eligible entry -- these cases are about the assembly behind it, whose second
    # workgroup has rows of its own only with 65 accepted entries or more)
    return _list(sc.round_csr_points_diverse(pts, strat, sel, 1.0, pool_size=pool, copy=True, boxes=boxes))


def call_tri(sc, inp, max_out, tri=None):
    sc.set_point(tri[2])
    ent, vio, nv = sc.tri_separate(max_out)
    return dict(entries=ent, violations=vio, n_violated=nv)


CALLS = {"select_round": call_select_round, "round_csr": call_round_csr, "begin_end": call_begin_end, "rank": call_rank,
         "skipped_round": call_skipped_round, "diverse": call_diverse, "multi": call_multi, "points": call_points,
         "points_diverse": call_points_diverse, "tri": call_tri}


def followup(sc, inp):
    """the fixed follow-up of three different calls: a fused select_round under another strategy at a new point, a round_csr with
    a head of 65 or more, score + rank -> one flat dict (the route statistics of the fused round included)"""
    out = {}
    direct = sc.get_stat(_capi.STAT_DIRECT_SELECTIONS)
    sc.set_point(inp["points"]["new"])
    for k, v in _copy(sc.select_round(2, 300)).items():
        out["sr." + k] = v
    out["sr.direct"] = sc.get_stat(_capi.STAT_DIRECT_SELECTIONS) - direct      # (the route this round took, not the handle's history)
    for k, v in _copy(sc.round_csr(1, 130, point=inp["points"]["weak"], copy=True)).items():
        out["csr." + k] = v
    sc.set_point(inp["points"]["strong"])
    sc.score(_capi.EIG | _capi.NN)
    out["eig"], out["obj"] = sc.get_scores()
    idx, score, n_total, new_strat, cnt = sc.rank(4, 200, max_out=200)
    out.update({"rank.idx": idx, "rank.score": score, "rank.n_total": n_total, "rank.new_strat": new_strat, "rank.counters": cnt})
    return out


def same(a, b, what):
    """byte equality of two flat result dicts"""
    assert sorted(a) == sorted(b), (what, sorted(set(a) ^ set(b)))
    for k in sorted(a):
        va, vb = a[k], b[k]
        if isinstance(va, np.ndarray):
            assert isinstance(vb, np.ndarray) and va.shape == vb.shape and va.dtype == vb.dtype and va.tobytes() == vb.tobytes(), (what, k)
        else:
            assert va == vb, (what, k, va, vb)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def _case(cid, site, inp, call, kw, consumers, first=0, count=1, injected=None, fallbacks=1, stats=None, error=None, against=None,
          tri=None, premise=None):
    return dict(id=cid, site=site, inputs=inp, call=call, kw=kw, consumers=tuple(consumers), first=first, count=count,
                injected=count if injected is None else injected, fallbacks=fallbacks, stats=stats or {}, error=error, against=against,
                tri=tri, premise=premise)


CASES = []
# S1: the fused rounds and the ranking on a void selection.  A fused round counts the give-up (round.hip: round_end) and answers by
# rank_on_device + emit_head; sdpcut_rank goes through rank_on_device alone, which counts nothing.
for _inp in ("generic", "nopf", "tie"):
    for _strat, _sel, _pt, _tag in ((1, 300, "gen", "s1"), (2, 300, "gen", "s2"), (4, 300, "strong", "s4strong"), (4, 300, "weak", "s4weak"),
                                    (6, 300, "gen", "s6")):
        if _inp == "tie" and _tag == "s4weak":
            continue      # four index sets: one point, whatever regime it is (sel below and above the strong count: on generic / nopf)
        _prem = {"s4strong": "strong_regime", "s4weak": "weak_regime"}.get(_tag)
        if _inp == "tie":
            _pt, _prem = "gen", "no_direct"
        for _call in ("select_round", "round_csr", "begin_end"):
            CASES.append(_case("S1-%s-%s-%s" % (_inp, _call, _tag), SELECT, _inp, _call, dict(strat=_strat, sel=_sel, point=_pt),
                               ("round.general_path", "rank.fast_finish", "rank.on_device"), premise=_prem))
        if _strat != 6:
            CASES.append(_case("S1-%s-rank-%s" % (_inp, _tag), SELECT, _inp, "rank", dict(strat=_strat, sel=_sel, point=_pt),
                               ("rank.fast_finish", "rank.on_device"), fallbacks=0, premise=_prem))
# S2: the skipped / filtered combined round
CASES.append(_case("S2-skipped-round", SELECT, "skip", "skipped_round", dict(strat=4, sel=300), ("round.skipped_void",),
                   stats={"nn_completions": 1}, premise="skipped"))
# S3: the exact head gives up to the ordinary round: equal to the OPTION-OFF round, not counted as a selection fallback
for _strat in (2, 4):
    CASES.append(_case("S3-exact-head-s%d" % _strat, SELECT, "exact", "round_csr", dict(strat=_strat, sel=300, point="strong"),
                       ("round.exact_gives_up",), fallbacks=0, stats={"exact_gave_up": 1}, against="exact_off", premise="exact"))
# S4: tri_separate
for _tri, _inp in (("golden20", "n20"), ("random40", "n40")):
    CASES.append(_case("S4-tri-%s-once" % _tri, SELECT, _inp, "tri", dict(max_out=5000), ("tri.relaunch",), tri=_tri, premise="tri"))
    CASES.append(_case("S4-tri-%s-twice" % _tri, SELECT, _inp, "tri", dict(max_out=5000), ("tri.relaunch",), count=2, tri=_tri,
                       error="tri_separate: selection void"))
# S5: the tie split whose own first selection is void (the round's own selection passes)
for _call in ("round_csr", "select_round"):
    CASES.append(_case("S5-tie-split-%s" % _call, SELECT, "vertex", _call, dict(strat=4, sel=500, point="gen"),
                       ("topk.tie_split_void", "round.general_path", "rank.on_device"), first=1, stats={"tie_splits": 0}, premise="tie_split"))
# L1: the fast path's enqueued assembly: csr_head_again(.., 1); count_failure = false -- the second give-up is not counted
for _inp, _heads in (("generic", (65, 129, 5000)), ("mixed", (65, 129, 142))):
    for _strat in (1, 4):
        for _h in _heads:
            _kw = dict(strat=_strat, sel=_h, point="strong" if (_strat == 4 and _inp == "generic") else "gen")
            CASES.append(_case("L1-%s-s%d-head%d-once" % (_inp, _strat, _h), LOOKBACK, _inp, "round_csr", _kw,
                               ("round.csr_head_again", "round.csr_assemble_wait"), premise="head"))
            CASES.append(_case("L1-%s-s%d-head%d-twice" % (_inp, _strat, _h), LOOKBACK, _inp, "round_csr", _kw,
                               ("round.csr_head_again", "round.csr_assemble_wait"), count=2, fallbacks=1, premise="head",
                               error="round_csr: look-back of the row assembly timed out twice"))
# L2: emit_head of the general path: a head beyond 8192 under the combined strategy (no fast attempt), and the every-entry-visited
# regime with SDPCUT_OPT_FUSE_KEYS = 0 and the regime resolved by the host.  csr_head_again(.., 2), count_failure = false: the first
# give-up is counted, the second is not.
CASES.append(_case("L2-big-head-once", LOOKBACK, "generic", "round_csr", dict(strat=4, sel=9000, point="gen"), ("round.csr_assemble_wait",)))
CASES.append(_case("L2-big-head-twice", LOOKBACK, "generic", "round_csr", dict(strat=4, sel=9000, point="gen"), ("round.csr_assemble_wait",),
                   count=2, fallbacks=1, error="round_csr: look-back of the row assembly timed out twice"))
# (nofuse: launch 1 of the site is the assembly enqueued behind the host-resolved STRONG attempt, whose head the host discards:
# first = 1 lets it pass and hits emit_head's)
CASES.append(_case("L2-every-entry-visited-once", LOOKBACK, "nofuse", "round_csr", dict(strat=4, sel=300, point="weak"),
                   ("round.csr_assemble_wait",), first=1, premise="weak_regime"))
CASES.append(_case("L2-every-entry-visited-twice", LOOKBACK, "nofuse", "round_csr", dict(strat=4, sel=300, point="weak"),
                   ("round.csr_assemble_wait",), first=1, count=2, fallbacks=1, premise="weak_regime",
                   error="round_csr: look-back of the row assembly timed out twice"))
# L3: the diverse round: csr_assemble_wait(.., 2, count_failure = true): both give-ups are counted
for _strat in (1, 6):
    CASES.append(_case("L3-diverse-s%d-once" % _strat, LOOKBACK, "generic", "diverse", dict(strat=_strat, sel=200),
                       ("round.csr_assemble_wait",), premise="head"))
    CASES.append(_case("L3-diverse-s%d-twice" % _strat, LOOKBACK, "generic", "diverse", dict(strat=_strat, sel=200),
                       ("round.csr_assemble_wait",), count=2, fallbacks=2, premise=None,
                       error="round_csr_diverse: look-back of the row assembly timed out twice"))
# L4: the multi-cut round with a quota that falls inside an entry (header word 11; row 70 is the second row of an entry of the
# second workgroup, by numpy's eigenvalues of the ranking's head -- asserted on the device's: quota_inside); count_failure = true
CASES.append(_case("L4-multi-once", LOOKBACK, "generic", "multi", dict(strat=1, sel=300, quota=70), ("round.csr_assemble_wait",),
                   premise="quota_inside"))
CASES.append(_case("L4-multi-twice", LOOKBACK, "generic", "multi", dict(strat=1, sel=300, quota=70), ("round.csr_assemble_wait",),
                   count=2, fallbacks=2, error="round_csr_multi: look-back of the row assembly timed out twice"))
# L5: the batched rounds: one fallback per point that went round again (fallbacks = "points": the points with a head, from handle A);
# the second give-up is the error and adds nothing
for _call, _kw, _cons, _what in (("points", dict(strat=1, sel=129), "points.again", "round_csr_points"),
                                 ("points", dict(strat=4, sel=129, boxed=True), "points.again", "round_csr_points"),
                                 ("points_diverse", dict(strat=1, sel=80, pool=320), "points.diverse_again", "round_csr_points_diverse"),
                                 ("points_diverse", dict(strat=6, sel=80, pool=320, boxed=True), "points.diverse_again", "round_csr_points_diverse")):
    _tag = "%s-s%d%s" % (_call, _kw["strat"], "-boxed" if _kw.get("boxed") else "")
    CASES.append(_case("L5-%s-once" % _tag, LOOKBACK, "spar020", _call, _kw, (_cons,), fallbacks="points", premise="points"))
    CASES.append(_case("L5-%s-twice" % _tag, LOOKBACK, "spar020", _call, _kw, (_cons,), count=2, fallbacks="points", premise="points",
                       error=_what + ": look-back of the row assembly timed out twice"))
# S6 (sharded; driven by test_gpu_giveup.py itself -- it needs torch's buffers): named here so that the table covers its consumers
SHARD_CASES = (
    dict(id="S6-world1-s1", strat=1, sel=300, consumers=("shard.void_record", "distributed.unfused")),
    dict(id="S6-world1-s2", strat=2, sel=300, consumers=("shard.void_record", "distributed.unfused")),
    dict(id="S6-ragged-shard0", strat=1, sel=300, consumers=("shard.void_record", "distributed.unfused")),
)

BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


def covered_consumers():
    out = set()
    for c in CASES:
        out.update(c["consumers"])
    for c in SHARD_CASES:
        out.update(c["consumers"])
    return out


# ---- the runner -------------------------------------------------------------------------------------------------------------------------
_FOLLOWUP_REF = {}


def followup_reference(lib, inp, tri_name):
    """the follow-up on a fresh handle, computed once per setup and shared"""
    key = (inp["name"], tuple(sorted(inp["options"].items())), tri_name)
    if key not in _FOLLOWUP_REF:
        sc = new_handle(lib, inp, tri_inputs(tri_name) if tri_name else None)
        try:
            _FOLLOWUP_REF[key] = followup(sc, inp)
        finally:
            sc.close()
    return _FOLLOWUP_REF[key]


def _stats(sc):
    out = {name: sc.get_stat(code) for name, code in STAT_NAMES.items()}
    out["injected"] = sc.get_stat(_capi.STAT_INJECTED)
    out["fallbacks"] = sc.get_stat(FB)
    return out


def check_premise(case, sc_a, res_a, inp, kw):
    """what the case supposes about its input, asserted on the undisturbed handle"""
    prem = case["premise"]
    if prem in ("strong_regime", "weak_regime"):
        sc_a.set_point(inp["points"][kw["point"]])
        sc_a.score(_capi.EIG | _capi.NN)
        eig, obj = sc_a.get_scores()
        n_strong = int(((obj > 0) & (eig < -1e-15)).sum())
        assert (n_strong >= kw["sel"]) == (prem == "strong_regime"), (prem, n_strong)
    elif prem == "no_direct":
        assert sc_a.get_stat(_capi.STAT_DIRECT_SELECTIONS) == 0
    elif prem == "skipped":      # the undisturbed round skipped, stayed in the strong regime and completed nothing
        assert sc_a.get_stat(_capi.STAT_NN_SKIPPED) > 0 and sc_a.get_stat(_capi.STAT_NN_COMPLETIONS) == 0
        assert res_a["new_strat"] == 4 and res_a["idx"].shape[0] == kw["sel"] and inp["ks"].shape[0] > 65536
    elif prem == "exact":
        assert sc_a.get_stat(_capi.STAT_EXACT_HEAD) == 1
    elif prem == "tie_split":
        assert sc_a.get_stat(_capi.STAT_TIE_SPLITS) == 1 and sc_a.get_stat(FB) == 0
    elif prem == "head":
        assert res_a["idx"].shape[0] > 0 and kw["sel"] >= 65
    elif prem == "tri":
        assert res_a["n_violated"] > 0 and res_a["entries"].shape[0] > 0
    elif prem == "quota_inside":
        assert res_a["quota_hit"] and res_a["rhs"].shape[0] == kw["quota"] and res_a["row_rank"][-1] < res_a["n_neg"][res_a["row_entry"][-1]] - 1
    elif prem == "points":
        heads = [res_a["p%d.idx" % p].shape[0] for p in range(8)]
        assert max(heads) >= 65 and sum(1 for w in heads if w > 0) >= 2, heads


def run_case(lib, case, report=None):
    inp = get_inputs(lib, case["inputs"])
    tri = tri_inputs(case["tri"]) if case["tri"] else None
    kw = dict(case["kw"])
    if tri is not None:
        kw["tri"] = tri
    call = CALLS[case["call"]]
    a = new_handle(lib, get_inputs(lib, case["against"]) if case["against"] else inp, tri)
    b = new_handle(lib, inp, tri)
    try:
        res_a = call(a, inp, **kw)
        if case["against"]:      # the premise is about the case's own setup, undisturbed
            p = new_handle(lib, inp, tri)
            try:
                check_premise(case, p, call(p, inp, **kw), inp, kw)
            finally:
                p.close()
        else:
            check_premise(case, a, res_a, inp, kw)
        want_fb = case["fallbacks"]
        if want_fb == "points":
            want_fb = sum(1 for p in range(8) if res_a["p%d.idx" % p].shape[0] > 0)
        before = _stats(b)
        b.set_option(_capi.OPT_INJECT_GIVEUP, _capi.inject_giveup(case["site"], case["first"], case["count"]))
        if case["error"]:
            try:
                call(b, inp, **kw)
            except _capi.SdpCutError as e:
                assert case["error"] in str(e), str(e)
            else:
                raise AssertionError("the call returned; expected: " + case["error"])
            assert b.pending is None
            b.set_option(_capi.OPT_SKIP_NONVIOLATED, b_skip(inp))      # refused with SDPCUT_ESTATE if a round were pending
            if case["call"] in ("points", "points_diverse") and kw.get("boxed"):
                assert b.box is None
        else:
            res_b = call(b, inp, **kw)
            same(res_a, res_b, case["id"])
            if kw.get("boxed"):
                assert b.box is None
        after = _stats(b)
        moved = {k: after[k] - before[k] for k in after}
        if report is not None:
            report("%-44s injected %d  fallbacks %d  %s" % (case["id"], moved["injected"], moved["fallbacks"],
                                                          "  ".join("%s %+d" % (k, moved[k]) for k in sorted(case["stats"]))))
        assert moved["injected"] == case["injected"], moved
        assert moved["fallbacks"] == want_fb, (moved, want_fb)
        ref_stats = _stats(a)
        for name, delta in case["stats"].items():
            # the amount beyond what the undisturbed call itself moves the statistic by (a fresh handle: its value on A)
            base = 0 if case["against"] else ref_stats[name]
            assert moved[name] - base == delta, (name, moved[name], base, delta)
        if case["premise"] == "exact":
            assert b.get_stat(_capi.STAT_EXACT_HEAD) == 0
        if case["premise"] == "skipped":      # the measure the round completed on its way: a plain score(EIG | NN) of a fresh handle
            p = new_handle(lib, inp, tri)
            try:
                p.set_point(inp["points"]["strong"])
                p.score(_capi.EIG | _capi.NN)
                want = p.get_scores()
            finally:
                p.close()
            got = b.get_scores()
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
            assert b.get_stat(_capi.STAT_NN_COMPLETIONS) == after["nn_completions"]
        # the follow-up, on the same handle
        mid = _stats(b)
        same(followup_reference(lib, inp, case["tri"]), followup(b, inp), case["id"] + " follow-up")
        end = _stats(b)
        assert end["injected"] == mid["injected"] and end["fallbacks"] == mid["fallbacks"], (mid, end)
        if tri is not None:      # the separation again, undisturbed, and with the fused tail still on
            same(res_a, call(b, inp, **kw), case["id"] + " again")
            assert b.get_stat(FB) == end["fallbacks"]
    finally:
        a.close()
        b.close()


def b_skip(inp):
    return inp["options"].get(_capi.OPT_SKIP_NONVIOLATED, 1)
