"""A handle on a caller's stream: the helpers and the case table of test_stream_cases_cpu.py (the table alone, no GPU) and
test_gpu_streams.py (the device).  A plain module: no fixtures, no GPU and no torch at import.

The contract ("Streams"; include/sdpcut.h at sdpcut_set_stream): all work of a handle runs on ITS stream --
its own non-blocking one, or the caller's after sdpcut_set_stream --, a switch orders the new stream behind everything the handle has
enqueued on the old one, and device pointers handed to the library are read and written in the handle's stream order.  A caller's
stream changes ordering, never results, so every case is held, byte for byte, against a fresh handle on its own stream
(tests/op_sequences.py: Fixtures, Model, new_handle, the operations).

Delays.  `delay(stream, ms)` keeps a stream busy with torch.cuda._sleep; the cycles per millisecond are measured once per process
(median of three event pairs), no clock is assumed.  50 ms where a case asserts a premise ("the producer had not finished when the
call returned"), 5 ms in part A, where the call under test waits for its result anyway.  50 ms is a choice, not a measurement: it
has to outlast a few host calls of microseconds, and the premise assertion says so when it does not.

Poison.  What a missing dependency would read too early, or leave unwritten, must show as wrong numbers and never as a fault:
  * caller-owned VALUE buffers (the LP point, score and measure outputs) are pre-filled with NaN, id outputs that only a clone()
    reads with -1;
  * nothing that a kernel uses as an address is ever poisoned.  The handle's own arrays cannot be reached from a test, so they are
    "poisoned" with VALID stale data: the scores, the LP point and the box tables of ANOTHER point / box (POISON_POINT,
    POISON_BOX), set and synchronised beforehand -- a consumer that runs ahead ranks the other point's scores, in bounds;
  * a gathered shard record carries ids the rows kernel addresses by, so its buffer is pre-filled with the valid record of the
    other point, not with a pattern.

The control.  Whether a missing dependency between two streams can show at all depends on the hardware queues the two land on.
`racing_pair()` looks for a pair of torch streams on which a dependent copy demonstrably runs ahead of a delayed fill; part D's
torch-to-torch cases run on that pair and skip when none of MAX_PAIRS pairs races (nothing else skips).

CASES has one entry per row of the four parts:
  A  every call family of op_sequences on a caller's stream (a torch side stream, the NULL stream);
  B  device-side producers: the LP point arrives by a copy on the caller's stream, sdpcut_set_point_device reads it in order;
  C  device-side consumers: outputs in caller-owned tensors are complete for the caller's next operation on the stream;
  D  hand-over: work enqueued on one stream, sdpcut_set_stream, the dependent call on another.
`entries` are the entry points of include/sdpcut.h with a device-pointer or stream parameter that the row exercises; `no_wait`
those entry points, returning without a host wait, whose premise the row asserts when they return."""
import numpy as np

import op_sequences as S
from sdpcutsel_via_nn_amd import _capi

DELAY_MS = 50
SHORT_DELAY_MS = 5
MAX_PAIRS = 8

POINT = "gen"               # the LP point every case of B, C and D computes at
POISON_POINT = "weak"       # the stale one
BOX, POISON_BOX = 1, 2
LIST = "E"                  # 5000 candidates of 2..5 variables: every network, the launch over all classes
TAIL_LIST = "D"             # 40000: a ranking of more than 16384 entries keeps its tail on the device
STREAM_KINDS = ("side", "null")
TARGETS = ("torch", "own", "null")

# the entry points that enqueue and return without a host wait (DESIGN.md "Streams" gives the same list; the CPU test compares)
NO_WAIT = ("sdpcut_score", "sdpcut_set_point", "sdpcut_set_point_device", "sdpcut_wake", "sdpcut_round_csr_begin",
           "sdpcut_merge_topk_device", "sdpcut_gather_scores_device", "sdpcut_shard_head_device", "sdpcut_shard_finish_enqueue")


# ---- delays and the control --------------------------------------------------------------------------------------------------------
_state = {"cycles_per_ms": None, "pair": None, "pair_log": []}


def cycles_per_ms():
    """torch.cuda._sleep cycles per millisecond on this device: median of three event pairs around a fixed spin"""
    if _state["cycles_per_ms"] is None:
        import torch
        spin = 2000000
        torch.cuda._sleep(spin)          # (the first launch loads the kernel)
        torch.cuda.synchronize()
        rates = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(spin)
            b.record()
            b.synchronize()
            rates.append(spin / a.elapsed_time(b))
        _state["cycles_per_ms"] = sorted(rates)[1]
    return _state["cycles_per_ms"]


def delay(stream, ms):
    """occupy `stream` (a torch stream; torch.cuda.default_stream() is the NULL stream) for about `ms` milliseconds"""
    import torch
    assert 0 < ms <= DELAY_MS
    cycles = int(ms * cycles_per_ms())
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)


def racing_pair():
    """-> (index, s1, s2): the first of MAX_PAIRS pairs of fresh torch streams on which a clone enqueued on s2 runs AHEAD of a
    fill enqueued earlier on s1 behind a delay; None when every pair was serialised (a shared hardware queue).  Looked for once per
    process; pair_log() says what each pair did."""
    if _state["pair"] is None:
        import torch
        cycles_per_ms()
        found = False
        for i in range(MAX_PAIRS):
            s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
            buf = torch.full((4096,), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            delay(s1, DELAY_MS)
            with torch.cuda.stream(s1):
                buf.fill_(1.0)
            with torch.cuda.stream(s2):
                out = buf.clone()
            torch.cuda.synchronize()
            out = out.cpu().numpy()
            raced = bool(np.isnan(out).all())
            _state["pair_log"].append((i, "raced" if raced else "serialised" if (out == 1.0).all() else "mixed"))
            if raced:
                _state["pair"] = (i, s1, s2)
                found = True
                break
        if not found:
            _state["pair"] = False
    return _state["pair"] or None


def pair_log():
    return list(_state["pair_log"])


# ---- part A: every operation of the alphabet, with the documented state it needs ---------------------------------------------------
A_FAMILIES = ("point",) + S.FAMILIES
A_LISTS = {"round": "C", "rank": TAIL_LIST}      # heads of 8192 and 9000 entries; a ranking with a tail on the device
# the cut pool is stateful by design: its operations run as one sequence on the handle under test and on its own-stream twin
POOL_SEQUENCE = ("pool/create", "pool/add", "pool/step", "pool/step_gen", "pool/step_weak", "pool/state", "pool/add", "pool/destroy")
PROBE = "round/csr4"        # run behind an operation that returns nothing (a setter), where the state allows a round


def family_ops(fam):
    return [name for name, op in S.OPS.items() if op["fam"] == fam]


def state_for(name):
    """-> (Model, scored): a documented state in which operation `name` is legal -- list, point, box, triangle table, training
    set, the exact measure for strategy 3, the begun round for round/end"""
    op = S.OPS[name]
    need = op.get("needs", ())
    m = S.Model()
    m.lst = "A" if op["fam"] == "list" else A_LISTS.get(op["fam"], LIST)
    m.point = POISON_POINT if "set_point" in op else POINT
    if "box" in need:
        m.box = BOX
    m.tri = "tri" in need
    m.train = "train" in need
    scored = 0
    if op.get("strat") == 3:
        m.opts["exact_sdp"] = 1
        scored = _capi.SDP
    if name == "score/get":      # the fetch of whatever is scored
        scored = _capi.EIG | _capi.NN
    if name == "round/end":
        m.pending = (4, 500)
    assert m.check(name) == "ok", (name, m.check(name))
    return m, scored


def probe_for(name, model_after):
    """the operation that makes a setter's effect visible: round/end behind a begun round, PROBE where a round is legal"""
    if model_after.pending is not None:
        return "round/end"
    return PROBE if model_after.check(PROBE) == "ok" else None


# ---- part B: operations behind sdpcut_set_point_device ------------------------------------------------------------------------------
def _scores(sc, fx):
    sc.score(_capi.EIG | _capi.NN)
    e, o = sc.get_scores()
    return dict(eig=e, obj=o)


def _efficacy(sc, fx):
    sc.score(_capi.EFF)
    eff, objpar, escore = sc.get_efficacy()
    return dict(eff=eff, objpar=objpar, escore=escore)


def _begin_end(sc, fx, probe=None):
    sc.round_csr_begin(4, 500)
    if probe is not None:
        probe("sdpcut_round_csr_begin")
    return S._round(sc.round_csr_end(copy=True))


def _objective(sc, fx):
    sc.set_objective(np.random.default_rng(5).normal(size=S.L_VARS + S.N_VARS))
    sc.set_efficacy_weight(0.1)


def _tri(sc, fx):
    sc.tri_preprocess(fx.adjacency)


def _pool(sc, fx):
    sc.pool_create(S.POOL_CAPACITY)
    sc.pool_add(*fx.pool_block)


# name -> (set-up on the handle before the point arrives, the operation)
B_OPS = {
    "score_eig_nn": (None, _scores),
    "score_eff": (_objective, _efficacy),
    "select_round_1": (None, lambda sc, fx: S._round(sc.select_round(1, 300))),
    "select_round_2": (None, lambda sc, fx: S._round(sc.select_round(2, 300))),
    "select_round_4": (None, lambda sc, fx: S._round(sc.select_round(4, 300))),
    "round_csr": (None, lambda sc, fx: S._round(sc.round_csr(4, 500, point=None, copy=True))),
    "round_csr_begin_end": (None, _begin_end),
    "round_csr_diverse": (None, lambda sc, fx: S._round(sc.round_csr_diverse(None, 4, 100, 0.5, copy=True))),
    "round_csr_multi": (None, lambda sc, fx: S._round(sc.round_csr_multi(None, 4, 200, 5, copy=True))),
    "tri_round_csr": (_tri, lambda sc, fx: sc.tri_round_csr(10000, point=None, copy=True)),
    "dense_round": (None, lambda sc, fx: S._round(sc.dense_round(None, copy=True))),
    "pool_step": (_pool, lambda sc, fx: sc.pool_step(point=None, max_age=1, drop_age=2, max_return=100, copy=True)),
}

# ---- part C: calls that write caller-owned device buffers ---------------------------------------------------------------------------
C_CALLS = {
    # name: (entry points, those of them that return without waiting)
    "rank_device": (("sdpcut_rank_device",), ()),      # (returns counts: it waits for its selection)
    "rank_device_efficacy": (("sdpcut_rank_device",), ()),      # strategy 6 against the stable sort of the device's own escore
    "gather_scores_device": (("sdpcut_gather_scores_device",), ("sdpcut_gather_scores_device",)),
    "merge_topk_device": (("sdpcut_merge_topk_device",), ("sdpcut_merge_topk_device",)),
    "merge_topk_device_secondary": (("sdpcut_merge_topk_device",), ("sdpcut_merge_topk_device",)),
    "shard_head_device": (("sdpcut_shard_head_device",), ("sdpcut_shard_head_device",)),
    # the gathered records arrive by a copy on the caller's stream behind a delay; the finish reads them in order
    "shard_finish_enqueue": (("sdpcut_shard_finish_enqueue",), ("sdpcut_shard_finish_enqueue",)),
    "shard_finish_round": (("sdpcut_shard_finish_round",), ()),
    "shard_finish_round_view": (("sdpcut_shard_finish_round_view",), ()),
    "shard_finish_round_own": (("sdpcut_shard_finish_round_own",), ()),
}
SHARD_COUNT, SHARD_SEL = 64, 32

# ---- part D: producer on s1, sdpcut_set_stream, consumer on the target --------------------------------------------------------------
# name: (list, producer's entry points, those whose premise -- not finished at the switch -- is asserted).  sdpcut_set_box and
# sdpcut_rank_device wait for the stream themselves in front of their last launches, so the delay is gone when they return and what
# they leave on the old stream is a tail of microseconds: no premise can hold there, and a pass proves little.
D_CASES = {
    "score__get_scores": (LIST, (), ("sdpcut_score",)),
    "score__rank": (LIST, (), ("sdpcut_score",)),
    "score__select_round": (LIST, (), ("sdpcut_score",)),
    "set_point_device__score": (LIST, ("sdpcut_set_point_device",), ("sdpcut_set_point_device",)),
    "set_point__round_csr": (LIST, (), ("sdpcut_set_point",)),      # the one sdpcut_set_stream has always handled (point_inflight)
    "set_box__score_nn": (LIST, (), ()),
    "wake__round_csr": (LIST, (), ("sdpcut_wake",)),
    "rank_device__rank_fetch": (TAIL_LIST, ("sdpcut_rank_device",), ()),
}


def _case(part, ident, entries=(), no_wait=(), **kw):
    kw.update(part=part, id=ident, entries=tuple(entries) + ("sdpcut_set_stream",), no_wait=tuple(no_wait))
    return kw


CASES = []
for _fam in A_FAMILIES:
    for _kind in STREAM_KINDS:
        CASES.append(_case("A", "A-%s-%s" % (_fam, _kind), family=_fam, kind=_kind,
                           ops=list(POOL_SEQUENCE) if _fam == "pool" else family_ops(_fam)))
for _name in B_OPS:
    for _box in (False, True):
        CASES.append(_case("B", "B-%s%s" % (_name, "-box" if _box else ""), ("sdpcut_set_point_device",),
                           ("sdpcut_set_point_device",) + (("sdpcut_round_csr_begin",) if _name == "round_csr_begin_end" else ()),
                           op=_name, box=_box))
for _name, (_entries, _nw) in C_CALLS.items():
    CASES.append(_case("C", "C-" + _name, _entries, _nw, call=_name))
for _target in TARGETS:
    for _name, (_lst, _entries, _nw) in D_CASES.items():
        CASES.append(_case("D", "D-%s-to-%s" % (_name, _target), _entries, _nw, case=_name, target=_target, lst=_lst))


def cases(part):
    return [c for c in CASES if c["part"] == part]
