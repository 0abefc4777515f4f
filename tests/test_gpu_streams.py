"""A handle on a caller's stream, held to stream order (tests/stream_cases.py holds the helpers, the poison rules and the case
table; DESIGN.md section 5 "Streams" and include/sdpcut.h at sdpcut_set_stream the contract).

Every comparison is byte for byte (`_same` of test_gpu_op_sequences.py) against a fresh handle on its own stream that is given its
inputs from the host and waited for after every call -- the way every other GPU test drives the library.

  A  every operation of op_sequences.OPS on a torch side stream and on the NULL stream, with 5 ms of foreign work enqueued in front
     of it: a launch, copy or event of the library that goes to the own or the null stream instead of h->stream shows here.
  B  the LP point arrives in a NaN-filled tensor by a copy on the caller's stream behind 50 ms; sdpcut_set_point_device and every
     call family that reads the point must see it.  Premise: the copy had not finished when sdpcut_set_point_device returned.
  C  the calls that write caller-owned device buffers: a clone() enqueued on the caller's stream right behind the call, with no
     host synchronisation in between, holds the complete result.
  D  work enqueued on s1 behind 50 ms, sdpcut_set_stream, the dependent call on another stream.  Between two torch streams the
     cases run on the pair stream_cases.racing_pair() found to race -- the control: on that pair a missing dependency shows -- and
     skip when no pair races.  From s1 to the handle's own stream and to the NULL stream there is no control (the own stream cannot
     be given to torch): a pass there may be vacuous.
  E  sdpcut_set_stream with the stream the handle already has changes nothing; SDPCUT_STAT_SELECT_FALLBACKS stays 0 throughout.

Nothing here is meant to fault: whatever a missing dependency would read is valid stale data or NaN in a value buffer
(stream_cases.py, "Poison"), and every handle is closed only after the whole device has been waited for."""
import ctypes
import time

import numpy as np
import pytest

import op_sequences as S
import stream_cases as sc_
from test_gpu_op_sequences import _call, _same

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    import sdpcutsel_via_nn_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def torch():
    import torch
    torch.cuda.set_device(0)
    print("torch.cuda._sleep: %.0f cycles per millisecond" % sc_.cycles_per_ms())
    return torch


@pytest.fixture(scope="module")
def fx():
    return S.Fixtures()


@pytest.fixture(scope="module")
def side(torch):
    """the caller's side stream of parts A to C and E"""
    return torch.cuda.Stream()


@pytest.fixture(scope="module")
def d_points(torch, fx):
    """the two LP points on the device, there before anything is timed"""
    pts = {name: torch.from_numpy(fx.point(name)).cuda() for name in (sc_.POINT, sc_.POISON_POINT)}
    torch.cuda.synchronize()
    return pts


def _capi():
    from sdpcutsel_via_nn_amd import _capi
    return _capi


def _close(h, torch):
    """nothing of a handle is freed while a stream may still hold work that touches it"""
    torch.cuda.synchronize()
    if h.pending is not None:
        h.drop_pending()
    h.close()


def _no_fallbacks(h, where):
    n = h.get_stat(_capi().STAT_SELECT_FALLBACKS)
    assert n == 0, "%s: SDPCUT_STAT_SELECT_FALLBACKS is %d" % (where, n)


def _kind_stream(kind, torch, side):
    """-> (torch stream, what sdpcut_set_stream takes)"""
    return (torch.cuda.default_stream(), 0) if kind == "null" else (side, side.cuda_stream)


def _try(fn, *args, **kw):
    try:
        return "ok", fn(*args, **kw)
    except (ValueError, _capi().SdpCutError) as e:
        return type(e).__name__, str(e)


def _same_steps(got, ref, where):
    assert [g[:2] for g in got] == [r[:2] for r in ref], "%s: %s, the fresh handle on its own stream %s" % (
        where, [g[:2] + ((g[2],) if g[1] != "ok" else ()) for g in got], [r[:2] + ((r[2],) if r[1] != "ok" else ()) for r in ref])
    for (label, status, out), (_, _, out_ref) in zip(got, ref):
        if status == "ok":
            _same(out, out_ref, "%s, %s" % (where, label))


def _premise(flags, where):
    for entry, held in flags.items():
        assert held, ("%s: premise not met -- the work in front of %s had finished when the call returned, so the %d ms delay was "
                      "too short to show anything" % (where, entry, sc_.DELAY_MS))


def _not_done(stream, torch):
    """an event recorded behind everything enqueued on `stream` so far is not complete yet"""
    ev = torch.cuda.Event()
    ev.record(stream)
    return not ev.query()


# ---- calibration and the control --------------------------------------------------------------------------------------------------
def test_delay_is_calibrated(torch, side):
    """the delay helper really occupies a stream for about what it is asked for (the premise assertions rest on it)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(side)
    sc_.delay(side, sc_.DELAY_MS)
    b.record(side)
    b.synchronize()
    ms = a.elapsed_time(b)
    print("a delay of %d ms took %.1f ms at %.0f cycles per millisecond" % (sc_.DELAY_MS, ms, sc_.cycles_per_ms()))
    assert 0.5 * sc_.DELAY_MS <= ms <= 2.0 * sc_.DELAY_MS


def test_control_pair_is_reported(torch):
    pair = sc_.racing_pair()
    print("racing_pair: %s; pairs tried: %s" % ("pair %d races" % pair[0] if pair else "no pair raced", sc_.pair_log()))
    assert len(sc_.pair_log()) >= 1 and (pair is None) == all(what != "raced" for _, what in sc_.pair_log())


# ---- A: every call family on a caller's stream --------------------------------------------------------------------------------------
def _run_op(lib, fx, torch, name, stream, ptr):
    """operation `name` on a handle made for it (stream None: on its own stream) -> [(label, status, result)]: the operation,
    SDPCUT_STAT_SCORED behind it, and behind an operation that returns nothing the probe that shows its effect"""
    capi = _capi()
    model, scored = sc_.state_for(name)
    op = S.OPS[name]
    h = S.new_handle(lib, fx, model, scored)
    try:
        if stream is not None:
            h.set_stream(ptr)
            sc_.delay(stream, sc_.SHORT_DELAY_MS)
        ctx = {"rows": None}
        status, out = _call(op, h, model, fx, ctx)
        steps = [(name, status, out)]
        if status == "ok":
            model.apply(name)
            if model.pending is None:
                steps.append(("SDPCUT_STAT_SCORED", "ok", h.get_stat(capi.STAT_SCORED)))
            probe = sc_.probe_for(name, model) if out == {} else None
            if probe is not None:
                if stream is not None:
                    sc_.delay(stream, sc_.SHORT_DELAY_MS)
                steps.append((probe,) + _call(S.OPS[probe], h, model, fx, ctx))
        if stream is not None:
            _no_fallbacks(h, name)
        return steps
    finally:
        _close(h, torch)


def _run_pool(lib, fx, torch, stream, ptr):
    capi = _capi()
    model = S.Model()
    model.lst, model.point = sc_.LIST, sc_.POINT
    h = S.new_handle(lib, fx, model)
    try:
        if stream is not None:
            h.set_stream(ptr)
        steps, ctx = [], {"rows": None}
        for name in sc_.POOL_SEQUENCE:
            assert model.check(name) == "ok", name
            if stream is not None:
                sc_.delay(stream, sc_.SHORT_DELAY_MS)
            steps.append((name,) + _call(S.OPS[name], h, model, fx, ctx))
            model.apply(name)
            steps.append(("SDPCUT_STAT_SCORED after " + name, "ok", h.get_stat(capi.STAT_SCORED)))
        if stream is not None:
            _no_fallbacks(h, "the pool sequence")
        return steps
    finally:
        _close(h, torch)


@pytest.fixture(scope="module")
def own_stream_results(lib, fx, torch):
    """each operation on a fresh handle on its own stream, run once and shared by the stream kinds"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run_pool(lib, fx, torch, None, None) if name == "pool" else _run_op(lib, fx, torch, name, None, None)
        return cache[name]
    return get


@pytest.mark.parametrize("case", sc_.cases("A"), ids=lambda c: c["id"])
def test_family_on_a_callers_stream(lib, fx, torch, side, own_stream_results, case):
    stream, ptr = _kind_stream(case["kind"], torch, side)
    t0 = time.perf_counter()
    if case["family"] == "pool":
        _same_steps(_run_pool(lib, fx, torch, stream, ptr), own_stream_results("pool"), case["id"])
    else:
        for name in case["ops"]:
            _same_steps(_run_op(lib, fx, torch, name, stream, ptr), own_stream_results(name), "%s, operation %s" % (case["id"], name))
    print("%s: %d operations, %.2f s" % (case["id"], len(case["ops"]), time.perf_counter() - t0))


# ---- B: the LP point produced on the caller's stream ------------------------------------------------------------------------------
def _run_b(lib, fx, torch, side, d_points, name, box, device):
    setup, fn = sc_.B_OPS[name]
    model = S.Model()
    model.lst, model.box = sc_.LIST, (sc_.BOX if box else None)
    model.point = sc_.POISON_POINT if device else sc_.POINT
    h = S.new_handle(lib, fx, model)
    flags = {}
    try:
        if setup is not None:
            setup(h, fx)
        kw = {}
        if device:
            h.synchronize()
            h.set_stream(side.cuda_stream)
            p = torch.full((S.L_VARS + S.N_VARS,), NAN, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            sc_.delay(side, sc_.DELAY_MS)
            with torch.cuda.stream(side):
                p.copy_(d_points[sc_.POINT], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
            h.set_point_device(p.data_ptr())
            flags["sdpcut_set_point_device"] = not ev.query()
            if name == "round_csr_begin_end":
                kw["probe"] = lambda entry: flags.__setitem__(entry, _not_done(side, torch))
        status, out = _try(fn, h, fx, **kw)
        if device:
            _no_fallbacks(h, name)
        return [(name, status, out), ("SDPCUT_STAT_SCORED", "ok", h.get_stat(_capi().STAT_SCORED))], flags
    finally:
        _close(h, torch)


@pytest.fixture(scope="module")
def host_point_results(lib, fx, torch):
    cache = {}

    def get(name, box):
        if (name, box) not in cache:
            cache[(name, box)] = _run_b(lib, fx, torch, None, None, name, box, False)[0]
        return cache[(name, box)]
    return get


@pytest.mark.parametrize("case", sc_.cases("B"), ids=lambda c: c["id"])
def test_point_produced_on_the_callers_stream(lib, fx, torch, side, d_points, host_point_results, case):
    ref = host_point_results(case["op"], case["box"])
    got, flags = _run_b(lib, fx, torch, side, d_points, case["op"], case["box"], True)
    assert sorted(flags) == sorted(case["no_wait"])
    _premise(flags, case["id"])
    _same_steps(got, ref, case["id"])


# ---- C: results in caller-owned device buffers ------------------------------------------------------------------------------------
def _state_handle(lib, fx, point, scored):
    model = S.Model()
    model.lst, model.point = sc_.LIST, point
    return S.new_handle(lib, fx, model, scored)


@pytest.fixture(scope="module")
def c_refs(lib, fx, torch):
    """what the host twins return at the point of part C, each from a fresh handle on its own stream, and the two shard records"""
    capi = _capi()
    out = {}
    h = _state_handle(lib, fx, sc_.POINT, capi.EIG | capi.NN)
    try:
        out["eig"], out["obj"] = h.get_scores()
        idx, score, n_total, new_strat, cnt = h.rank(4, 500, max_out=500)
        out["rank"] = dict(idx=idx, score=score, n_total=n_total, new_strat=new_strat, counters=cnt)
        idx, score, _, _, _ = h.rank(2, 0, max_out=sc_.SHARD_COUNT)
        out["head2"] = dict(idx=idx, score=score)
    finally:
        _close(h, torch)
    from sdpcutsel_via_nn_amd import efficacy
    h = _state_handle(lib, fx, sc_.POINT, 0)
    try:
        sc_._objective(h, fx)
        h.score(capi.EFF)
        escore = h.get_efficacy()[2]
        order = efficacy.ranking(escore)[:500]
        out["rank6"] = dict(idx=order.astype(np.int64) + S.LISTS[sc_.LIST], score=escore[order], n_total=S.LIST_LENGTHS[sc_.LIST], new_strat=6)
    finally:
        _close(h, torch)
    for key, point in (("record", sc_.POINT), ("poison_record", sc_.POISON_POINT)):
        h = _state_handle(lib, fx, point, 0)
        try:
            rec = torch.full((8 + 2 * sc_.SHARD_COUNT,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            h.shard_head_device(2, sc_.SHARD_COUNT, rec.data_ptr())
            h.synchronize()
            out[key] = rec
        finally:
            _close(h, torch)
    h = _state_handle(lib, fx, sc_.POINT, 0)
    try:
        out["finish"] = h.shard_finish_round(1, sc_.SHARD_COUNT, out["record"].data_ptr(), sc_.SHARD_SEL, copy=True)
    finally:
        _close(h, torch)
    h = _state_handle(lib, fx, sc_.POINT, 0)
    try:
        r = h.shard_finish_round_own(1, sc_.SHARD_COUNT, out["record"].data_ptr(), sc_.SHARD_SEL)
        out["finish_own"] = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in r.items()}
    finally:
        _close(h, torch)
    assert not np.array_equal(out["record"].cpu().numpy(), out["poison_record"].cpu().numpy())
    return out


def _merge_inputs(secondary):
    rng = np.random.default_rng(6 if secondary else 5)
    n = 3000 if secondary else 4000
    scores = rng.integers(0, 20, n).astype(np.float64)       # many ties
    sec = rng.integers(-5, 5, n).astype(np.float64) if secondary else None
    ids = rng.permutation(10 ** 6)[:n].astype(np.int64)
    order = np.lexsort((ids, -sec, -scores)) if secondary else np.lexsort((ids, -scores))
    return scores, sec, ids, order[:n if secondary else 500]


def _raw_finish_round(h, d_allrec, world, count, sel):
    """sdpcut_shard_finish_round itself (the binding's shard_finish_round goes through the _view form)"""
    ld = h.row_len
    hdr, idx, ks = np.zeros((world, 8), dtype=np.int64), np.zeros(sel, dtype=np.int64), np.zeros(sel, dtype=np.int32)
    score, lam, rhs, coef = np.zeros(sel), np.zeros(sel), np.zeros(sel), np.zeros((sel, ld))
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    h._check(h._lib.sdpcut_shard_finish_round(h._h, world, count, ctypes.c_void_p(d_allrec), sel, ld, hdr.ctypes.data_as(ip),
                                             idx.ctypes.data_as(ip), score.ctypes.data_as(dp), lam.ctypes.data_as(dp),
                                             coef.ctypes.data_as(dp), rhs.ctypes.data_as(dp), ks.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    return dict(headers=hdr, idx=idx, score=score, lam=lam, coef=coef, rhs=rhs, ks=ks)


@pytest.mark.parametrize("case", sc_.cases("C"), ids=lambda c: c["id"])
def test_results_in_the_callers_buffers(lib, fx, torch, side, c_refs, case):
    capi = _capi()
    call = case["call"]
    unscored = call.startswith("shard_")
    h = _state_handle(lib, fx, sc_.POINT, 0 if unscored else capi.EIG | capi.NN)
    flags = {}

    def f64(n):
        return torch.full((n,), NAN, dtype=torch.float64, device="cuda")

    def i64(n):
        return torch.full((n,), -1, dtype=torch.int64, device="cuda")

    def clones(*tensors):
        with torch.cuda.stream(side):
            c = [t.clone() for t in tensors]
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in c]

    def returned(entry):
        if entry in case["no_wait"]:
            flags[entry] = _not_done(side, torch)

    try:
        h.synchronize()
        h.set_stream(side.cuda_stream)
        if call == "rank_device":
            d_idx, d_sc = i64(500), f64(500)
            torch.cuda.synchronize()
            sc_.delay(side, sc_.DELAY_MS)
            w, n_total, new_strat, cnt = h.rank_device(4, 500, 500, d_idx.data_ptr(), d_sc.data_ptr())
            idx, score = clones(d_idx, d_sc)
            _same(dict(idx=idx[:w], score=score[:w], n_total=n_total, new_strat=new_strat, counters=cnt), c_refs["rank"], case["id"])
        elif call == "rank_device_efficacy":
            sc_._objective(h, fx)
            h.score(capi.EFF)
            h.synchronize()
            d_idx, d_sc = i64(500), f64(500)
            torch.cuda.synchronize()
            sc_.delay(side, sc_.DELAY_MS)
            w, n_total, new_strat, cnt = h.rank_device(6, 0, 500, d_idx.data_ptr(), d_sc.data_ptr())
            idx, score = clones(d_idx, d_sc)
            _same(dict(idx=idx[:w], score=score[:w], n_total=n_total, new_strat=new_strat), c_refs["rank6"], case["id"])
        elif call == "gather_scores_device":
            ids = fx.ids(sc_.LIST, 200) + S.LISTS[sc_.LIST]
            d_ids, d_e, d_o = torch.from_numpy(ids).cuda(), f64(ids.shape[0]), f64(ids.shape[0])
            torch.cuda.synchronize()
            sc_.delay(side, sc_.DELAY_MS)
            h.gather_scores_device(ids.shape[0], d_ids.data_ptr(), d_e.data_ptr(), d_o.data_ptr())
            returned("sdpcut_gather_scores_device")
            e, o = clones(d_e, d_o)
            _same(dict(eig=e, obj=o), dict(eig=c_refs["eig"][ids], obj=c_refs["obj"][ids]), case["id"])
        elif call.startswith("merge_topk_device"):
            scores, sec, ids, order = _merge_inputs(call.endswith("secondary"))
            d_s, d_i = torch.from_numpy(scores).cuda(), torch.from_numpy(ids).cuda()
            d_q = torch.from_numpy(sec).cuda() if sec is not None else None
            o_s, o_i = f64(order.shape[0]), i64(order.shape[0])
            torch.cuda.synchronize()
            sc_.delay(side, sc_.DELAY_MS)
            h.merge_topk_device(scores.shape[0], d_s.data_ptr(), d_i.data_ptr(), order.shape[0], o_s.data_ptr(), o_i.data_ptr(),
                                d_q.data_ptr() if d_q is not None else None)
            returned("sdpcut_merge_topk_device")
            s, i = clones(o_s, o_i)
            _same(dict(score=s, ids=i), dict(score=scores[order], ids=ids[order]), case["id"])
        elif call == "shard_head_device":
            rec = i64(8 + 2 * sc_.SHARD_COUNT)
            torch.cuda.synchronize()
            sc_.delay(side, sc_.DELAY_MS)
            h.shard_head_device(2, sc_.SHARD_COUNT, rec.data_ptr())
            returned("sdpcut_shard_head_device")
            got, = clones(rec)
            _same(got, c_refs["record"].cpu().numpy(), case["id"])
            # the record against the host twin: list length and entries written, then the scores and ids of sdpcut_rank's head
            assert got[0] == S.LIST_LENGTHS[sc_.LIST] and got[3] == sc_.SHARD_COUNT and got[4] == 0
            _same(dict(score=got[8:8 + sc_.SHARD_COUNT].view(np.float64), idx=got[8 + sc_.SHARD_COUNT:]), c_refs["head2"], case["id"])
        else:
            # the gathered records: a buffer that holds the VALID record of the other point (it carries ids the rows are addressed
            # by), overwritten with this point's record by a copy on the caller's stream behind the delay
            allrec = c_refs["poison_record"].clone()
            torch.cuda.synchronize()
            sc_.delay(side, sc_.DELAY_MS)
            with torch.cuda.stream(side):
                allrec.copy_(c_refs["record"], non_blocking=True)
            args = (1, sc_.SHARD_COUNT, allrec.data_ptr(), sc_.SHARD_SEL)
            if call == "shard_finish_enqueue":
                h.shard_finish_enqueue(*args)
                returned("sdpcut_shard_finish_enqueue")
                got = {k: np.array(v) for k, v in h.shard_finish_wait(own=False).items()}
                ref = c_refs["finish"]
            elif call == "shard_finish_round":
                got, ref = _raw_finish_round(h, allrec.data_ptr(), 1, sc_.SHARD_COUNT, sc_.SHARD_SEL), c_refs["finish"]
            elif call == "shard_finish_round_view":
                got, ref = h.shard_finish_round(*args, copy=True), c_refs["finish"]
            else:
                got = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in h.shard_finish_round_own(*args).items()}
                ref = c_refs["finish_own"]
            _same(got, ref, case["id"])
        assert sorted(flags) == sorted(case["no_wait"])
        _premise(flags, case["id"])
        _no_fallbacks(h, case["id"])
    finally:
        _close(h, torch)


# ---- D: hand-over between streams ---------------------------------------------------------------------------------------------------
def _run_d(lib, fx, torch, d_points, name, lst, s1, target):
    """the case on a handle in the stale state (scores, point and box of the OTHER point / box, synchronised); s1 None: everything
    on the handle's own stream -- the reference.  -> (result, premise held at the switch, the consumer returned while the producer
    still had not run)"""
    capi = _capi()
    both = capi.EIG | capi.NN
    gen = fx.point(sc_.POINT)
    model = S.Model()
    model.lst, model.point = lst, sc_.POISON_POINT
    if name == "set_box__score_nn":
        model.box = sc_.POISON_BOX
    h = S.new_handle(lib, fx, model, both)
    out = {}
    try:
        if name.startswith("score__") or name in ("set_box__score_nn", "wake__round_csr", "rank_device__rank_fetch"):
            h.set_point(gen)
        if name == "rank_device__rank_fetch":
            h.score(both)
            d_idx = torch.full((20000,), -1, dtype=torch.int64, device="cuda")
            d_sc = torch.full((20000,), NAN, dtype=torch.float64, device="cuda")
        h.synchronize()
        if s1 is not None:
            h.set_stream(s1.cuda_stream)
            torch.cuda.synchronize()
            sc_.delay(s1, sc_.DELAY_MS)
        # the producer, on s1
        if name.startswith("score__"):
            h.score(both)
        elif name == "set_point_device__score":
            h.set_point_device(d_points[sc_.POINT].data_ptr())
        elif name == "set_point__round_csr":
            h.set_point(gen)
        elif name == "set_box__score_nn":
            h.set_box(*fx.box(sc_.BOX))
        elif name == "wake__round_csr":
            h.wake()
        else:
            w, n_total, new_strat, cnt = h.rank_device(2, 100, 20000, d_idx.data_ptr(), d_sc.data_ptr())
            out.update(w=w, n_total=n_total, new_strat=new_strat, counters=cnt)
        premise = ahead = None
        if s1 is not None:
            ev = torch.cuda.Event()
            ev.record(s1)
            premise = not ev.query()
            h.set_stream(target)
        # the consumer, on the target
        if name == "score__get_scores":
            out["eig"], out["obj"] = h.get_scores()
        elif name == "score__rank":
            idx, score, n_total, new_strat, cnt = h.rank(4, 500, max_out=500)
            out.update(idx=idx, score=score, n_total=n_total, new_strat=new_strat, counters=cnt)
        elif name == "score__select_round":
            out.update(S._round(h.select_round(4, 300)))
        elif name == "set_point_device__score":
            h.score(both)
            out["eig"], out["obj"] = h.get_scores()
        elif name in ("set_point__round_csr", "wake__round_csr"):
            out.update(S._round(h.round_csr(4, 500, copy=True)))
        elif name == "set_box__score_nn":
            h.score(capi.NN)
            out["obj"] = h.get_scores(eig=False)[1]
        else:
            out["fetch_idx"], out["fetch_score"] = h.rank_fetch(out["n_total"] // 2, 64)
        if s1 is not None:
            ahead = not ev.query()
        torch.cuda.synchronize()
        if name == "rank_device__rank_fetch":
            out["head_idx"], out["head_score"] = d_idx.cpu().numpy()[:out["w"]], d_sc.cpu().numpy()[:out["w"]]
        out["SDPCUT_STAT_SCORED"] = h.get_stat(capi.STAT_SCORED)
        if s1 is not None:
            _no_fallbacks(h, name)
        return out, premise, ahead
    finally:
        _close(h, torch)


@pytest.fixture(scope="module")
def d_refs(lib, fx, torch, d_points):
    cache = {}

    def get(name, lst):
        if name not in cache:
            cache[name] = _run_d(lib, fx, torch, d_points, name, lst, None, None)[0]
        return cache[name]
    return get


def _hand_over(lib, fx, torch, d_points, d_refs, case, s1, target):
    ref = d_refs(case["case"], case["lst"])
    got, premise, ahead = _run_d(lib, fx, torch, d_points, case["case"], case["lst"], s1, target)
    print("%s: premise %s; the consumer %s" % (case["id"], "held" if premise else "NOT met (the producer had finished at the switch)",
                                              "returned before the producer had run" if ahead else "returned behind the producer"))
    if case["no_wait"]:
        _premise({case["no_wait"][0]: premise}, case["id"])
    _same(got, ref, case["id"])


@pytest.mark.parametrize("case", [c for c in sc_.cases("D") if c["target"] == "torch"], ids=lambda c: c["id"])
def test_hand_over_between_torch_streams(lib, fx, torch, d_points, d_refs, case):
    """s1 -> s2 of the pair racing_pair() found: on it a dependent copy demonstrably runs ahead of delayed work, so a switch that
    does not order the new stream behind the old one returns the stale point's numbers here"""
    pair = sc_.racing_pair()
    if pair is None:
        pytest.skip("no pair of %d pairs of torch streams raced (%s): a missing dependency could not show" % (sc_.MAX_PAIRS, sc_.pair_log()))
    _, s1, s2 = pair
    _hand_over(lib, fx, torch, d_points, d_refs, case, s1, s2.cuda_stream)


@pytest.mark.parametrize("case", [c for c in sc_.cases("D") if c["target"] != "torch"], ids=lambda c: c["id"])
def test_hand_over_to_the_own_and_the_null_stream(lib, fx, torch, side, d_points, d_refs, case):
    """s1 -> SDPCUT_OWN_STREAM and s1 -> NULL.  No control: the handle's own stream cannot be given to torch, so whether the two
    streams of a case could race at all is not known, and a pass here may be vacuous."""
    _hand_over(lib, fx, torch, d_points, d_refs, case, side, None if case["target"] == "own" else 0)


# ---- E: what must not change --------------------------------------------------------------------------------------------------------
def _run_e(lib, fx, torch, ptr, redundant):
    """a short life of a handle on stream `ptr`; redundant: sdpcut_set_stream with that same stream in front of every call"""
    capi = _capi()
    model = S.Model()
    model.lst, model.point = sc_.LIST, sc_.POISON_POINT
    h = S.new_handle(lib, fx, model, capi.EIG | capi.NN)

    def again():
        if redundant:
            h.set_stream(ptr)
    try:
        h.synchronize()
        h.set_stream(ptr)
        again()
        h.set_point(fx.point(sc_.POINT))
        again()
        h.score(capi.EIG | capi.NN)
        again()
        out = {}
        out["eig"], out["obj"] = h.get_scores()
        again()
        out["round"] = S._round(h.round_csr(4, 500, copy=True))
        again()
        h.set_point(fx.point(sc_.POISON_POINT))
        again()
        out["fused_round"] = S._round(h.select_round(4, 300))
        out["SDPCUT_STAT_SCORED"] = h.get_stat(capi.STAT_SCORED)
        _no_fallbacks(h, "set_stream with the same stream")
        return out
    finally:
        _close(h, torch)


@pytest.mark.parametrize("kind", ("own",) + sc_.STREAM_KINDS)
def test_set_stream_with_the_same_stream_changes_nothing(lib, fx, torch, side, kind):
    ptr = None if kind == "own" else _kind_stream(kind, torch, side)[1]
    _same(_run_e(lib, fx, torch, ptr, True), _run_e(lib, fx, torch, ptr, False), "stream kind " + kind)
