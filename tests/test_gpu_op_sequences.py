"""Call sequences on ONE handle against a fresh handle per operation (tests/op_sequences.py holds the model, the alphabet and the
sequences; DESIGN.md section 5 "Call history" the contract).

The handle under test lives through a whole sequence.  Before every operation the test reads S = SDPCUT_STAT_SCORED on it; the
reference for that operation is a Scorer made for it and brought into the model's state -- networks, options, instance, list,
triangle table, training set, box, point, score(S) (the cut rows are documented to depend on the scored measures: with lambda_min
at hand the eigenvector comes from inverse iteration with it, include/sdpcut.h: sdpcut_cut_rows), a begun round -- on which the same
function runs.  Every array of the two results must have the same shape, dtype and BYTES (NaN padding and -0.0 count), every
integer must be equal, a refusal must be the same error class on both, and the operation after a refusal must agree again.
SDPCUT_STAT_SCORED after the operation must agree too; SDPCUT_STAT_NN_SKIPPED / _NN_EVALUATED are compared where the operation
entered with nothing scored and left the network's measure scored.  The cut pool is stateful by design: its operations run on the
handle under test and on a second long-lived handle that sees nothing but set_instance and the pool calls.

Anchor: the head of every rank / select_round / round_csr operation must also equal oracle.rank_arrays on the device's scores at
that (list, point, networks, box, kernel variant), fetched once from a fresh handle: ids, scores, n_total, new_strat and the strong
/ violated counters, bit for bit (the rule of test_gpu_fuzz.py).  Heads under SDPCUT_OPT_EXACT_HEAD are ordered by other bits
(tests/test_gpu_exact_head.py pins those) and are compared with the fresh handle only.

A sequence that fails is reduced by hand to the shortest prefix and pair that still fails and kept in op_sequences.HAND_SEQUENCES
under a name that says what it shows."""
import time

import numpy as np
import pytest

import op_sequences as S

pytestmark = pytest.mark.gpu

ROUND_RESULTS = ("indptr", "indices", "values", "rhs")


@pytest.fixture(scope="module")
def lib():
    import sdpcutsel_via_nn_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def fx():
    return S.Fixtures()


@pytest.fixture(scope="module")
def device_scores(lib, fx):
    """the device's scores per (list, point, networks, box, kernel variant), each fetched once from a fresh handle"""
    from sdpcutsel_via_nn_amd import _capi
    cache = {}

    def get(model, point, want_sdp):
        key = (model.lst, point, tuple(sorted(model.nets.items())), model.box, model.opts["kernel"])
        if key not in cache or (want_sdp and "sdp" not in cache[key]):
            m = S.Model()
            m.lst, m.point, m.nets, m.box = model.lst, point, dict(model.nets), model.box
            m.opts["kernel"] = model.opts["kernel"]
            sc = S.new_handle(lib, fx, m, _capi.EIG | _capi.NN)
            try:
                eig, obj = sc.get_scores()
                cache[key] = dict(eig=eig, obj=obj)
                if want_sdp:
                    sc.score(_capi.SDP)
                    cache[key]["sdp"] = sc.get_sdp_scores()[0]
            finally:
                sc.close()
        return cache[key]
    return get


def _first_difference(a, b):
    a8 = np.ascontiguousarray(a).reshape(-1).view(np.uint8).reshape(a.size, a.dtype.itemsize)
    b8 = np.ascontiguousarray(b).reshape(-1).view(np.uint8).reshape(b.size, b.dtype.itemsize)
    pos = int(np.flatnonzero((a8 != b8).any(axis=1))[0])
    return pos, a.reshape(-1)[pos], b.reshape(-1)[pos]


def _same(got, ref, where, field=""):
    """got (handle under test) against ref (fresh handle): dicts of arrays, ints and flat dicts"""
    if isinstance(ref, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(ref), "%s: fields %s against %s" % (where, sorted(got), sorted(ref))
        for k in ref:
            _same(got[k], ref[k], where, field + ("." if field else "") + str(k))
    elif isinstance(ref, np.ndarray):
        assert isinstance(got, np.ndarray) and got.shape == ref.shape and got.dtype == ref.dtype, \
            "%s: field %s is %s %s, the fresh handle gives %s %s" % (where, field, got.dtype, got.shape, ref.dtype, ref.shape)
        if got.tobytes() != ref.tobytes():
            pos, x, y = _first_difference(got, ref)
            raise AssertionError("%s: field %s differs first at position %d: %r, the fresh handle gives %r" % (where, field, pos, x, y))
    else:
        assert type(got) is type(ref) and got == ref, "%s: field %s is %r, the fresh handle gives %r" % (where, field, got, ref)


def _call(op, sc, model, fx, ctx):
    from sdpcutsel_via_nn_amd import _capi
    try:
        return "ok", op["fn"](sc, model, fx, ctx, **op["kw"])
    except (ValueError, _capi.SdpCutError) as e:
        return type(e).__name__, str(e)


def _check_oracle(oracle, device_scores, fx, model, name, op, res, where):
    """the head against oracle.rank_arrays on the device's own scores"""
    if name == "round/end":
        strat, sel = model.pending
        max_out = None
    else:
        strat, sel, max_out = op["kw"]["strat"], op["kw"]["sel"], op["kw"].get("max_out")
    if model.opts["exact_head"] and strat in (2, 4):
        return
    point = op["kw"].get("point") or model.point
    sco = device_scores(model, point, strat == 3)
    N, base = S.LIST_LENGTHS[model.lst], S.LISTS[model.lst]
    order, ref_score, ref_strat, ref_cnt = oracle.rank_arrays(2 if strat == 3 else strat, sco["sdp"] if strat == 3 else sco["obj"],
                                                              sco["eig"], sel)
    w = min(max_out if max_out is not None else sel, N, order.shape[0])
    assert res["idx"].shape[0] == w, "%s: head of %d entries, the oracle's has %d" % (where, res["idx"].shape[0], w)
    for field, got, ref in (("idx", res["idx"], order[:w] + base), ("score", res["score"], ref_score[:w] + 0.0)):
        if not np.array_equal(got, ref):
            pos = int(np.flatnonzero(got != ref)[0])
            raise AssertionError("%s: field %s differs from the oracle's ranking of the device's scores first at position %d: %r != %r"
                                 % (where, field, pos, got[pos], ref[pos]))
    assert res["n_total"] == order.shape[0], "%s: n_total %d, oracle %d" % (where, res["n_total"], order.shape[0])
    assert res["new_strat"] == (3 if strat == 3 else ref_strat), "%s: new_strat %d, oracle %d" % (where, res["new_strat"], ref_strat)
    if strat == 4:
        got = (res["counters"]["strong"], res["counters"]["violated"])
        assert got == (ref_cnt["strong"], ref_cnt["violated"]), "%s: strong / violated counters %r, oracle %r" % (where, got, ref_cnt)


def run_sequence(seq_name, lib, fx, oracle, device_scores):
    from sdpcutsel_via_nn_amd import _capi
    tokens = S.SEQUENCES[seq_name]
    model = S.Model()
    sut = S.new_handle(lib, fx, model)
    mirror = None        # the pool's second long-lived handle
    ctx = {"rows": None}
    begin_scored = 0
    prev = "(start)"
    try:
        for i, tok in enumerate(tokens):
            marked, name = S.parse(tok)
            op = S.OPS[name]
            where = "sequence %s, operation %d %s (after %s)" % (seq_name, i, tok, prev)
            verdict = model.check(name)
            assert verdict in ("ok", "refused") and marked == (verdict == "refused"), "%s: the model says %s" % (where, verdict)
            pending = model.pending is not None
            scored = begin_scored if pending else sut.get_stat(_capi.STAT_SCORED)
            if op["fam"] == "pool":
                if mirror is None:
                    mirror = lib.Scorer(0)
                    mirror.set_instance(S.N_VARS, fx.Q)
                status_ref, out_ref = _call(op, mirror, model, fx, dict(ctx, mirror=True))
                status, out = _call(op, sut, model, fx, ctx)
                assert status == status_ref, "%s: %s (%s), the pool's own handle %s (%s)" % (where, status, out, status_ref, out_ref)
                assert (status != "ok") == marked, "%s: %s (%s)" % (where, status, out)
                if status == "ok":
                    _same(out, out_ref, where)
            else:
                ref = S.new_handle(lib, fx, model, scored)
                try:
                    status_ref, out_ref = _call(op, ref, model, fx, ctx)
                    status, out = _call(op, sut, model, fx, ctx)
                    assert status == status_ref, "%s: %s (%s), the fresh handle %s (%s)" % (where, status, out, status_ref, out_ref)
                    assert (status != "ok") == marked, "%s: %s (%s)" % (where, status, out)
                    if status == "ok":
                        _same(out, out_ref, where)
                        if op.get("anchor"):
                            _check_oracle(oracle, device_scores, fx, model, name, op, out, where)
                        if not pending and not op.get("begins"):
                            after, after_ref = sut.get_stat(_capi.STAT_SCORED), ref.get_stat(_capi.STAT_SCORED)
                            assert after == after_ref, "%s: SDPCUT_STAT_SCORED %d afterwards, the fresh handle %d" % (where, after, after_ref)
                            entered = 0 if "set_point" in op else scored
                            if entered == 0 and (after & _capi.NN):
                                for stat, what in ((_capi.STAT_NN_SKIPPED, "NN_SKIPPED"), (_capi.STAT_NN_EVALUATED, "NN_EVALUATED")):
                                    a, b = sut.get_stat(stat), ref.get_stat(stat)
                                    assert a == b, "%s: SDPCUT_STAT_%s %d, the fresh handle %d" % (where, what, a, b)
                        if all(k in out for k in ROUND_RESULTS):
                            ctx["rows"] = tuple(out[k].copy() for k in ROUND_RESULTS)
                finally:
                    if ref.pending is not None:
                        ref.drop_pending()
                    ref.close()
            if op.get("begins") and status == "ok":
                begin_scored = scored
            if verdict == "ok":
                model.apply(name)
            prev = tok
    finally:
        if sut.pending is not None:
            sut.drop_pending()
        sut.close()
        if mirror is not None:
            mirror.close()


@pytest.mark.parametrize("name", sorted(S.SEQUENCES))
def test_sequence_against_fresh_handles(lib, fx, oracle, device_scores, name):
    t0 = time.perf_counter()
    run_sequence(name, lib, fx, oracle, device_scores)
    print("sequence %s: %d operations, %.2f s" % (name, len(S.SEQUENCES[name]), time.perf_counter() - t0))


def test_points_put_the_lists_in_their_regimes(lib, fx, device_scores):
    """the regimes the sequences count on, from the device's own scores: the strong point resolves STRONG for heads up to 5000 on C
    and D, the weak point makes every combined round visit every entry, nothing is violated at the PSD point, the structured vertex
    is full of ties -- and a combined round on C with SDPCUT_OPT_SKIP_NONVIOLATED = 2 takes the skipping launch"""
    from sdpcutsel_via_nn_amd import _capi
    m = S.Model()
    smallest_combined_head = min(op["sel"] for op in S.OPS.values() if op.get("strat") == 4)
    for lst in ("C", "D"):
        m.lst = lst
        sco = device_scores(m, "strong", False)
        assert int(((sco["obj"] > 0) & (sco["eig"] < -1e-15)).sum()) >= 5000, lst
        sco = device_scores(m, "weak", False)
        assert int(((sco["obj"] > 0) & (sco["eig"] < -1e-15)).sum()) < smallest_combined_head, lst
        sco = device_scores(m, "mid", False)
        assert np.unique(sco["eig"]).shape[0] < S.LIST_LENGTHS[lst] // 4, lst
    for lst in S.LISTS:
        m.lst = lst
        assert not (device_scores(m, "psd", False)["eig"] < -1e-15).any(), lst
        assert (device_scores(m, "gen", False)["eig"] < -1e-15).sum() > S.LIST_LENGTHS[lst] // 2, lst
    m.lst, m.point = "C", "strong"
    m.opts["skip"] = 2
    sc = S.new_handle(lib, fx, m)
    try:
        r = sc.round_csr(4, 5000, copy=True)
        nv = r["counters"]["nb_violated"]
        assert r["new_strat"] == 4 and r["counters"]["strong"] == 5000
        assert sc.get_stat(_capi.STAT_NN_SKIPPED) == S.LIST_LENGTHS["C"] - nv > 0
        assert 5000 <= sc.get_stat(_capi.STAT_NN_EVALUATED) <= nv
    finally:
        sc.close()
