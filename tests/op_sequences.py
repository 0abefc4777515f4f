"""Call sequences on one handle: the state model, the alphabet of operations and the committed sequences of
test_op_sequences_cpu.py (the model alone, no GPU) and test_gpu_op_sequences.py (one long-lived handle against a fresh handle per
operation).  A plain module: no fixtures, no GPU.

The contract the sequences enforce ("Call history"): apart from the cut pool the result of a call is a
function of the instance, the candidate list, the networks, the options, the node box, the LP point and the measures scored at
that point -- never of the calls before it.  `Model` carries exactly that documented state; `new_handle` builds a handle in
that state from nothing.

Alphabet: every operation is a function (scorer, model, fixtures, ctx) -> dict of numpy arrays, ints and flat dicts of ints, named
"family/variant" in OPS; the same function drives the handle under test and its reference.  The 15 families that pairs are drawn
from are FAMILIES; `point` (set_point) is the sixteenth, the separator of the pair coverage.  ROUND_LIKE are the families whose
operations run a selection round; every ordered pair of families with a round-like member is covered twice, adjacent and with one
`point` operation in between (adjacent keeps the scored measures of X alive into Y).

Left out on purpose: the sharded calls (sdpcut_shard_*, rank_device, merge / gather on device buffers -- they need a second
runtime's buffers and a process group), set_stream (a caller's stream changes ordering, not results, and needs torch:
stream_cases.py / test_gpu_streams.py run this alphabet on a caller's stream, and the device-pointer calls in stream order),
SDPCUT_OPT_INJECT_GIVEUP (test only; it changes no result either, and giveup_cases.py / test_gpu_giveup.py run it against fresh
handles in the same way -- LEFT_OUT_OPTIONS below names it, and the model's statistics list knows SDPCUT_STAT_INJECTED),
SDPCUT_OPT_COOP_LAUNCH (another way to launch the same selection kernel: it changes no result and no state a later call reads) and
SDPCUT_OPT_SIDE_STREAMS = 2, which picks a code path from a timing.

Sequences are data: lists of operation names, "!" in front of one the model expects the library to refuse (the handle must stay
usable).  PAIR_* cover the family pairs, HAND_* the adjacencies the library's own comments name, RANDOM_* are four seeded walks of
60 operations under the model's preconditions.

Fields compared under a rule other than byte equality: none.  Not compared at all (they depend on history or on what else runs on
the device): SDPCUT_STAT_ROUNDS, _SELECT_FALLBACKS, _TIE_SPLITS, _NN_COMPLETIONS, the _PF_* diagnostics and last_timing;
SDPCUT_STAT_NN_SKIPPED and _NN_EVALUATED only after an operation that entered with nothing scored and left the network's measure
scored."""
import itertools

import numpy as np

from sdpcutsel_via_nn_amd import _capi, networks, synthetic

N_VARS = 40
INSTANCE_SEED = 7
L_VARS = N_VARS * (N_VARS + 1) // 2

FAMILIES = ("score", "rank", "round", "rows", "diverse", "multi", "points", "box", "dense", "tri", "batch", "pool", "list", "net", "option")
ROUND_LIKE = ("round", "diverse", "multi", "points", "box", "dense")

# option name -> (id, default, documented values)
OPTIONS = {
    "skip": (_capi.OPT_SKIP_NONVIOLATED, 1, (0, 1, 2)),
    "fp32": (_capi.OPT_FP32_FILTER, 1, (0, 1)),
    "count_rank": (_capi.OPT_COUNT_RANK, 1, (0, 1)),
    "fuse_keys": (_capi.OPT_FUSE_KEYS, 1, (0, 1)),
    "fused_tail": (_capi.OPT_FUSED_TAIL, 1, (0, 1)),
    "auto_regime": (_capi.OPT_AUTO_REGIME, 1, (0, 1)),
    "kernel": (_capi.OPT_KERNEL, _capi.KERNEL_MFMA, (_capi.KERNEL_MFMA, _capi.KERNEL_VALU)),
    "exact_head": (_capi.OPT_EXACT_HEAD, 0, (0, 1)),
    "one_launch": (_capi.OPT_ONE_LAUNCH, 1, (0, 1)),
    "prefilter": (_capi.OPT_PREFILTER, 1, (0, 1)),
    "exact_sdp": (_capi.OPT_EXACT_SDP, 0, (0, 1)),
}
# options of the header that the alphabet leaves out on purpose (the docstring says why), and the statistics a comparison skips
LEFT_OUT_OPTIONS = {"inject_giveup": _capi.OPT_INJECT_GIVEUP, "coop_launch": _capi.OPT_COOP_LAUNCH, "side_streams": _capi.OPT_SIDE_STREAMS,
                    "timing": _capi.OPT_TIMING, "eig_kernel": _capi.OPT_EIG_KERNEL, "stream_priority": _capi.OPT_STREAM_PRIORITY}
HISTORY_STATS = {"rounds": _capi.STAT_ROUNDS, "select_fallbacks": _capi.STAT_SELECT_FALLBACKS, "tie_splits": _capi.STAT_TIE_SPLITS,
                 "nn_completions": _capi.STAT_NN_COMPLETIONS, "injected": _capi.STAT_INJECTED}
# name -> global_base (Fixtures.list says what each list is for)
LISTS = {"A": 0, "B": 7, "C": 0, "D": 10 ** 9, "E": 0}
LIST_LENGTHS = {"A": 130, "B": 6000, "C": 9880, "D": 40000, "E": 5000}
POINTS = ("gen", "strong", "weak", "mid", "psd")
NETS = {3: ("ship", "speaks", "heard", "both"), 4: ("ship", "user")}
BATCH_POINTS = ("gen", "strong", "mid")
EXACT_HEAD_LIMIT = 8192      # TK_LDSK: head plus band of a round under SDPCUT_OPT_EXACT_HEAD
POOL_CAPACITY = 16384
POOL_ADD_ROWS = 200


# ---- fixtures: instance, lists, points, networks, boxes, the fixed input block ---------------------------------------------------
class Fixtures(object):
    """everything the operations read, made once and never changed"""

    def __init__(self):
        self.Q, _, _ = synthetic.make_instance(N_VARS, INSTANCE_SEED)
        self._lists, self._points, self._nets, self._boxes = {}, {}, {}, {}
        self.adjacency = np.ones((N_VARS, N_VARS), dtype=np.uint8) - np.eye(N_VARS, dtype=np.uint8)      # 4 T = 39 520 entries
        import user_nets
        self.block = user_nets.nn_batch_inputs(3, seed=5, count=257)      # rows [x | q] of nn_batch / sdp_batch / train_set_data
        rng = np.random.default_rng(11)
        self.targets = rng.uniform(-1.0, 0.0, self.block.shape[0])
        self.eig_x = np.ascontiguousarray(self.block[:, :3])
        self.eig_X = rng.uniform(0.0, 1.0, (self.block.shape[0], 6)) * np.minimum.reduce(
            [self.eig_x[:, [0, 0, 0, 1, 1, 2]], self.eig_x[:, [0, 1, 2, 1, 2, 2]]])
        # rows for a pool that no round has fed yet: x_i - X_ii >= 0 on the first variables
        m = 8
        diag = N_VARS * np.arange(m) - np.arange(m) * (np.arange(m) - 1) // 2
        self.pool_block = (np.arange(0, 2 * m + 1, 2, dtype=np.int32),
                           np.stack([L_VARS + np.arange(m), diag], axis=1).ravel().astype(np.int32),
                           np.tile([1.0, -1.0], m), np.zeros(m))

    def list(self, name):
        """-> (set_inds int32 [N, 5] padded with -1, ks int32 [N], global_base)"""
        if name not in self._lists:
            n = N_VARS
            if name == "A":      # one-workgroup select-and-sort route
                ks = np.full(130, 4, dtype=np.int32)
                sets = synthetic.random_index_sets(n, 4, 130, np.random.default_rng(201))
            elif name == "B":    # TK_ROUTE_SMALLSEL window; repeated sets give exact ties
                ks = np.full(6000, 3, dtype=np.int32)
                sets = synthetic.random_index_sets(n, 3, 6000, np.random.default_rng(202))
            elif name == "C":    # all triples: the list of test_gpu_skip_nonviolated.py
                sets = np.array(list(itertools.combinations(range(n), 3)), dtype=np.int32)
                ks = np.full(sets.shape[0], 3, dtype=np.int32)
            elif name == "D":    # above SDPCUT_PF_MIN_N; about four copies of each triple
                ks = np.full(40000, 3, dtype=np.int32)
                sets = synthetic.random_index_sets(n, 3, 40000, np.random.default_rng(204))
            elif name == "E":    # the launch over all classes; rows of every length
                rng = np.random.default_rng(205)
                ks = rng.choice([2, 3, 4, 5], size=5000).astype(np.int32)
                sets = None
            else:
                raise KeyError(name)
            pad = np.full((ks.shape[0], 5), -1, dtype=np.int32)
            if sets is None:
                for k in (2, 3, 4, 5):
                    sel = ks == k
                    pad[sel, :k] = synthetic.random_index_sets(n, k, int(sel.sum()), rng)
            else:
                pad[:, :sets.shape[1]] = sets
            assert pad.shape[0] == LIST_LENGTHS[name]
            self._lists[name] = (pad, ks, LISTS[name])
        return self._lists[name]

    def ids(self, name, count=40):
        """local candidate ids spread over the list, with one repeat"""
        N = LIST_LENGTHS[name]
        ids = np.unique(np.linspace(0, N - 1, min(N, count)).astype(np.int64))
        return np.concatenate([ids, ids[:1]])

    def point(self, name):
        """LP points [X packed | x]: the constructions of test_gpu_count_rank.py (gen / strong / weak; x of the strong point drawn
        from [0.3, 0.7], where the McCormick interval is wide enough for more than half of all triples to be strong) and of
        test_gpu_fuzz.py (mid / psd); seeds found on the CPU with the oracle, regimes asserted on the device's scores by
        test_gpu_op_sequences.py"""
        if name not in self._points:
            n, Q = N_VARS, self.Q
            rng = np.random.default_rng({"gen": 2, "strong": 1, "weak": 1, "mid": 0, "psd": 1}[name])
            iu = np.triu_indices(n)
            x = rng.uniform(0.3, 0.7, n) if name == "strong" else rng.uniform(0, 1, n)
            lo = np.maximum(0.0, x[iu[0]] + x[iu[1]] - 1.0)
            hi = np.minimum(x[iu[0]], x[iu[1]])
            if name == "psd":        # X = min(x_i, x_j): the lifted matrix is PSD, nothing violated
                X = hi
            elif name == "mid":      # structured vertex: many exactly equal scores
                x = np.full(n, 0.5)
                X = rng.choice([0.0, 0.5], size=iu[0].shape[0])
            else:
                u = rng.uniform(0, 0.2, lo.shape[0])
                t = rng.uniform(0, 1, lo.shape[0]) if name == "gen" else np.where((Q > 0) == (name == "weak"), 1 - u, u)
                X = lo + t * (hi - lo)
            self._points[name] = np.concatenate([X, x])
        return self._points[name]

    def points(self):
        return np.stack([self.point(p) for p in BATCH_POINTS])

    def net(self, k, name):
        if (k, name) not in self._nets:
            if name == "ship":
                net = networks.load_network(k)
            elif name == "user":
                import user_nets
                net = user_nets.unshaped_network(k)
            else:
                import filter_tail_nets
                net = filter_tail_nets.tail_network(name)
            self._nets[(k, name)] = net
        return self._nets[(k, name)]

    def box(self, seed):
        if seed not in self._boxes:
            import nodebox_cases
            self._boxes[seed] = nodebox_cases.random_box(N_VARS, seed)
        return self._boxes[seed]


# ---- the state model ---------------------------------------------------------------------------------------------------------------
class Model(object):
    """the documented state of a handle that has its instance: what a call's result may depend on"""

    def __init__(self):
        self.lst = None              # current list id
        self.point = None            # current point id
        self.point_dropped = False   # a batched call left the handle without a current point
        self.nets = {2: "ship", 3: "ship", 4: "ship", 5: "ship"}
        self.opts = {name: spec[1] for name, spec in OPTIONS.items()}
        self.box = None              # seed of the node box
        self.pool = False
        self.tri = False
        self.train = False
        self.pending = None          # (strat, sel_size) of a begun round

    def check(self, name):
        """-> "ok", "refused" (the library refuses the call by design and the handle stays as it is) or "illegal: why" (a
        sequence must not hold the operation here)"""
        op = OPS[name]
        need = op.get("needs", ())
        if self.pending is not None:
            if name == "round/end":
                return "ok"
            return "refused" if op.get("pending_refused") else "illegal: a round is pending"
        if name == "round/end":
            return "illegal: no round begun"
        for what, have in (("list", self.lst is not None), ("pool", self.pool), ("tri", self.tri), ("train", self.train),
                           ("box", self.box is not None)):
            if what in need and not have:
                return "illegal: no " + what
        if "point" in need and self.point is None:
            return "refused" if self.point_dropped else "illegal: no point"
        if op.get("nobox") and self.box is not None:
            return "refused"
        if "set_box" in op and self.opts["exact_head"]:
            return "refused"
        strat, sel = op.get("strat"), op.get("sel", 0)
        if strat == 3 and not self.opts["exact_sdp"]:
            return "refused"
        if op.get("head_limit") and self.opts["exact_head"] and strat in (2, 4):
            cap = min(sel, LIST_LENGTHS[self.lst])
            if cap > 0 and min(LIST_LENGTHS[self.lst], cap + max(256, cap // 8)) > EXACT_HEAD_LIMIT:
                return "refused"
        return "ok"

    def apply(self, name):
        op = OPS[name]
        if "set_point" in op:
            self.point, self.point_dropped = op["set_point"], False
        if op.get("drops_point"):
            self.point, self.point_dropped = None, True
        if "set_list" in op:
            self.lst = op["set_list"]
        if "set_net" in op:
            self.nets[op["set_net"][0]] = op["set_net"][1]
        if "set_opt" in op:
            self.opts[op["set_opt"][0]] = op["set_opt"][1]
        if "set_box" in op:
            self.box = op["set_box"]
        if "set_pool" in op:
            self.pool = op["set_pool"]
        if op.get("set_tri"):
            self.tri = True
        if op.get("set_train"):
            self.train = True
        if op.get("begins"):
            self.pending = (op["strat"], op["sel"])
        if name == "round/end":
            self.pending = None


def parse(token):
    """"!name" -> (True, name)"""
    return (True, token[1:]) if token.startswith("!") else (False, token)


def new_handle(lib, fx, model, scored=0):
    """a handle made for one operation, brought into the model's state: networks, options, instance, list, triangle table,
    training set, box, point, the measures `scored` at it, the begun round"""
    sc = lib.Scorer(0)
    try:
        for k in (2, 3, 4, 5):
            sc.set_network(k, *fx.net(k, model.nets[k]))
        for name in sorted(OPTIONS):
            sc.set_option(OPTIONS[name][0], model.opts[name])
        sc.set_instance(N_VARS, fx.Q)
        if model.lst is not None:
            sc.set_candidates(*fx.list(model.lst))
        if model.tri:
            sc.tri_preprocess(fx.adjacency)
        if model.train:
            sc.train_set_data(3, fx.block, fx.targets)
        if model.box is not None:
            sc.set_box(*fx.box(model.box))
        if model.point is not None:
            sc.set_point(fx.point(model.point))
        if scored:
            sc.score(scored)
        if model.pending is not None:
            sc.round_csr_begin(model.pending[0], model.pending[1])
    except Exception:
        sc.close()
        raise
    return sc


# ---- the operations ----------------------------------------------------------------------------------------------------------------
_NEED = {1: _capi.EIG, 2: _capi.NN, 3: _capi.SDP, 4: _capi.EIG | _capi.NN}


def _round(r):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}


def _pt(fx, point):
    return None if point is None else fx.point(point)


def op_point(sc, m, fx, ctx, point):
    sc.set_point(fx.point(point))
    return {}


def op_score(sc, m, fx, ctx, flags):
    if flags:
        sc.score(flags)
    S = sc.get_stat(_capi.STAT_SCORED)
    out = {"scored": S}
    if S & (_capi.EIG | _capi.NN):
        e, o = sc.get_scores(eig=bool(S & _capi.EIG), obj=bool(S & _capi.NN))
        if e is not None:
            out["eig"] = e
        if o is not None:
            out["obj"] = o
    if S & _capi.SDP:
        out["sdp"], out["gap"] = sc.get_sdp_scores()
    return out


def op_rank(sc, m, fx, ctx, strat, sel, max_out):
    missing = _NEED[strat] & ~sc.get_stat(_capi.STAT_SCORED)
    if missing:
        sc.score(missing)
    idx, score, n_total, new_strat, cnt = sc.rank(strat, sel, max_out=max_out)
    out = dict(idx=idx, score=score, n_total=n_total, new_strat=new_strat, counters=cnt)
    off = n_total // 2
    count = min(64, n_total - off)
    if count > 0:
        # a window behind the head; a ranking that came from the top-k selection has no tail on the device and refuses the fetch
        # (include/sdpcut.h: sdpcut_rank_fetch) -- which of the two it is must not depend on the history either
        try:
            out["fetch_idx"], out["fetch_score"] = sc.rank_fetch(off, count)
            out["tail"] = 1
        except _capi.SdpCutError:
            out["tail"] = 0
    return out


def op_select_round(sc, m, fx, ctx, strat, sel):
    return _round(sc.select_round(strat, sel))


def op_round_csr(sc, m, fx, ctx, strat, sel, point=None, view=False):
    r = sc.round_csr(strat, sel, point=_pt(fx, point), copy=not view)
    return _round(r)      # (a view is read completely here)


def op_begin(sc, m, fx, ctx, strat, sel):
    sc.round_csr_begin(strat, sel)
    return {}


def op_end(sc, m, fx, ctx):
    return _round(sc.round_csr_end(copy=True))


def op_cut_rows(sc, m, fx, ctx):
    lam, coef, rhs, cols, ks = sc.cut_rows(fx.ids(m.lst))
    return dict(lam=lam, coef=coef, rhs=rhs, cols=cols, ks=ks)


def op_cut_rows_all(sc, m, fx, ctx, per_set):
    row_ptr, lam, coef, rhs, cols, ks = sc.cut_rows_all(fx.ids(m.lst), per_set)
    return dict(row_ptr=row_ptr, lam=lam, coef=coef, rhs=rhs, cols=cols, ks=ks)


def op_diverse(sc, m, fx, ctx, strat, sel, max_parallel, point=None):
    r = _round(sc.round_csr_diverse(_pt(fx, point), strat, sel, max_parallel, copy=True))
    return r


def op_filter_parallel(sc, m, fx, ctx):
    keep, info = sc.filter_parallel(fx.ids(m.lst, 200), 50, 0.5)
    return dict(keep=keep, info=info)


def op_multi(sc, m, fx, ctx, strat, sel, per_set, quota, point=None):
    return _round(sc.round_csr_multi(_pt(fx, point), strat, sel, per_set, row_quota=quota, copy=True))


def op_score_points(sc, m, fx, ctx):
    e, o = sc.score_points(fx.points())
    return dict(eig=e, obj=o)


def op_round_points(sc, m, fx, ctx, strat, sel):
    out = {}
    for p, r in enumerate(sc.round_csr_points(fx.points(), strat, sel, copy=True)):
        for k, v in r.items():
            out["p%d.%s" % (p, k)] = v
    return out


def op_set_box(sc, m, fx, ctx, seed):
    sc.set_box(*fx.box(seed))
    return {}


def op_clear_box(sc, m, fx, ctx):
    sc.clear_box()
    return {}


def op_dense_round(sc, m, fx, ctx, point=None):
    return _round(sc.dense_round(_pt(fx, point), copy=True))


def op_dense_eig(sc, m, fx, ctx):
    w, v = sc.dense_eig(vectors=True)
    return dict(eigvals=w, vectors=v)


def op_tri_prep(sc, m, fx, ctx):
    tri, dens = sc.tri_preprocess(fx.adjacency)
    return dict(triples=tri, density=dens)


def op_tri_separate(sc, m, fx, ctx, max_out):
    ent, vio, nv = sc.tri_separate(max_out)
    return dict(entries=ent, violations=vio, n_violated=nv)


def op_nn_batch(sc, m, fx, ctx):
    return dict(out=sc.nn_batch(3, fx.block))


def op_eig_batch(sc, m, fx, ctx):
    w, v = sc.eig_batch(3, fx.eig_x, fx.eig_X, want_vectors=True)
    return dict(eigvals=w, vectors=v)


def op_sdp_batch(sc, m, fx, ctx):
    return sc.sdp_batch(3, fx.block, want_certificate=True)


def op_train_data(sc, m, fx, ctx):
    sc.train_set_data(3, fx.block, fx.targets)
    return {}


def op_train_loss(sc, m, fx, ctx, first, count):
    loss, grad = sc.train_loss_grad(3, *fx.net(3, "ship"), first=first, count=count)
    return dict(loss=np.array([loss]), grad=grad)


def op_pool_create(sc, m, fx, ctx):
    sc.pool_create(POOL_CAPACITY)
    return {}


def op_pool_add(sc, m, fx, ctx):
    """the CSR rows of the round before it (those of the handle under test, kept by the driver in ctx["rows"]); a fixed block
    where no round has produced rows yet"""
    rows = ctx.get("rows")
    if rows is None or rows[3].shape[0] == 0:
        rows = fx.pool_block
    indptr, indices, values, rhs = rows
    n = min(POOL_ADD_ROWS, rhs.shape[0])
    first = sc.pool_add(indptr[:n + 1], indices, values, rhs[:n])
    return dict(first_serial=first, n_rows=n)


def op_pool_step(sc, m, fx, ctx, point=None):
    if point is None and ctx.get("mirror"):      # the mirror handle sees no set_point: it gets the model's current point
        point = m.point
    return sc.pool_step(point=_pt(fx, point), max_age=1, drop_age=2, max_return=100, copy=True)


def op_pool_state(sc, m, fx, ctx):
    return sc.pool_state()


def op_pool_destroy(sc, m, fx, ctx):
    sc.pool_destroy()
    return {}


def op_set_list(sc, m, fx, ctx, name):
    sc.set_candidates(*fx.list(name))
    return {}


def op_set_net(sc, m, fx, ctx, k, name):
    sc.set_network(k, *fx.net(k, name))
    return {}


def op_set_option(sc, m, fx, ctx, name, value):
    sc.set_option(OPTIONS[name][0], value)
    return {}


def _op(fam, fn, kw=None, **spec):
    spec.update(fam=fam, fn=fn, kw=kw or {})
    return spec


LP = ("list", "point")
OPS = {}
for _p in POINTS:
    OPS["point/" + _p] = _op("point", op_point, dict(point=_p), set_point=_p)
OPS.update({
    # score: sdpcut_score and the fetches behind it
    "score/eig": _op("score", op_score, dict(flags=_capi.EIG), needs=LP, pending_refused=True),
    "score/nn": _op("score", op_score, dict(flags=_capi.NN), needs=LP),
    "score/both": _op("score", op_score, dict(flags=_capi.EIG | _capi.NN), needs=LP),
    "score/sdp": _op("score", op_score, dict(flags=_capi.SDP), needs=LP),
    "score/get": _op("score", op_score, dict(flags=0), needs=("list",)),      # get_scores of whatever is scored: completes a partial measure
    # rank: sdpcut_rank (scoring what the strategy misses) and a window of sdpcut_rank_fetch behind it
    "rank/1": _op("rank", op_rank, dict(strat=1, sel=0, max_out=300), needs=LP, strat=1, anchor=True),
    "rank/2": _op("rank", op_rank, dict(strat=2, sel=500, max_out=500), needs=LP, strat=2, sel=500, anchor=True),
    "rank/4": _op("rank", op_rank, dict(strat=4, sel=500, max_out=500), needs=LP, strat=4, sel=500, anchor=True),
    "rank/3": _op("rank", op_rank, dict(strat=3, sel=0, max_out=200), needs=LP, strat=3, anchor=True),
    "rank/big": _op("rank", op_rank, dict(strat=2, sel=100, max_out=20000), needs=LP, strat=2, sel=100, anchor=True),      # > 16 384: the full-list workspace
    # round: the fused rounds
    "round/sel1": _op("round", op_select_round, dict(strat=1, sel=300), needs=LP, strat=1, sel=300, head_limit=True, anchor=True),
    "round/sel2": _op("round", op_select_round, dict(strat=2, sel=300), needs=LP, strat=2, sel=300, head_limit=True, anchor=True),
    "round/sel4": _op("round", op_select_round, dict(strat=4, sel=300), needs=LP, strat=4, sel=300, head_limit=True, anchor=True),
    "round/sel4_5000": _op("round", op_select_round, dict(strat=4, sel=5000), needs=LP, strat=4, sel=5000, head_limit=True, anchor=True),
    "round/sel1_8192": _op("round", op_select_round, dict(strat=1, sel=8192), needs=LP, strat=1, sel=8192, head_limit=True, anchor=True),
    "round/sel2_8192": _op("round", op_select_round, dict(strat=2, sel=8192), needs=LP, strat=2, sel=8192, head_limit=True, anchor=True),
    "round/sel1_9000": _op("round", op_select_round, dict(strat=1, sel=9000), needs=LP, strat=1, sel=9000, head_limit=True, anchor=True),
    "round/sel4_9000": _op("round", op_select_round, dict(strat=4, sel=9000), needs=LP, strat=4, sel=9000, head_limit=True, anchor=True),
    "round/csr1": _op("round", op_round_csr, dict(strat=1, sel=500), needs=LP, strat=1, sel=500, head_limit=True, anchor=True),
    "round/csr2": _op("round", op_round_csr, dict(strat=2, sel=500), needs=LP, strat=2, sel=500, head_limit=True, anchor=True),
    "round/csr4": _op("round", op_round_csr, dict(strat=4, sel=500), needs=LP, strat=4, sel=500, head_limit=True, anchor=True),
    "round/csr3": _op("round", op_round_csr, dict(strat=3, sel=200), needs=LP, strat=3, sel=200, anchor=True),
    "round/csr4_5000": _op("round", op_round_csr, dict(strat=4, sel=5000), needs=LP, strat=4, sel=5000, head_limit=True, anchor=True),
    "round/view4": _op("round", op_round_csr, dict(strat=4, sel=500, view=True), needs=LP, strat=4, sel=500, head_limit=True, anchor=True),
    "round/csrpt_gen": _op("round", op_round_csr, dict(strat=4, sel=500, point="gen"), needs=("list",), strat=4, sel=500, set_point="gen",
                           anchor=True),
    "round/csrpt_strong": _op("round", op_round_csr, dict(strat=4, sel=500, point="strong"), needs=("list",), strat=4, sel=500,
                              set_point="strong", anchor=True),
    "round/csrpt_weak": _op("round", op_round_csr, dict(strat=1, sel=500, point="weak"), needs=("list",), strat=1, sel=500,
                            set_point="weak", anchor=True),
    "round/begin4": _op("round", op_begin, dict(strat=4, sel=500), needs=LP, strat=4, sel=500, head_limit=True, begins=True),
    "round/begin1": _op("round", op_begin, dict(strat=1, sel=500), needs=LP, strat=1, sel=500, begins=True),
    "round/end": _op("round", op_end, anchor=True),
    # rows
    "rows/cut": _op("rows", op_cut_rows, needs=LP),
    "rows/all1": _op("rows", op_cut_rows_all, dict(per_set=1), needs=LP),
    "rows/all3": _op("rows", op_cut_rows_all, dict(per_set=3), needs=LP),
    # diverse
    "diverse/r1": _op("diverse", op_diverse, dict(strat=1, sel=100, max_parallel=0.5), needs=LP, strat=1, sel=100),
    "diverse/r4": _op("diverse", op_diverse, dict(strat=4, sel=100, max_parallel=0.5), needs=LP, strat=4, sel=100),
    "diverse/r2pt_gen": _op("diverse", op_diverse, dict(strat=2, sel=100, max_parallel=0.9, point="gen"), needs=("list",), strat=2, sel=100,
                            set_point="gen"),
    "diverse/filter": _op("diverse", op_filter_parallel, needs=LP),
    # multi: cuts_per_set 1 and 5, with and without a row quota of its own
    "multi/m1": _op("multi", op_multi, dict(strat=4, sel=200, per_set=1, quota=None), needs=LP, strat=4, sel=200, head_limit=True),
    "multi/m5": _op("multi", op_multi, dict(strat=4, sel=200, per_set=5, quota=None), needs=LP, strat=4, sel=200, head_limit=True),
    "multi/m5sets": _op("multi", op_multi, dict(strat=1, sel=200, per_set=5, quota="sets"), needs=LP, strat=1, sel=200),
    "multi/m1q50": _op("multi", op_multi, dict(strat=2, sel=200, per_set=1, quota=50), needs=LP, strat=2, sel=200, head_limit=True),
    "multi/m5pt_strong": _op("multi", op_multi, dict(strat=4, sel=200, per_set=5, quota=None, point="strong"), needs=("list",), strat=4,
                             sel=200, set_point="strong"),
    # points: P = 3 LP points per call (list A: the one-launch route; the longer lists: the loop)
    "points/score": _op("points", op_score_points, needs=("list",), nobox=True, drops_point=True, pending_refused=True),
    "points/round4": _op("points", op_round_points, dict(strat=4, sel=100), needs=("list",), nobox=True, drops_point=True, strat=4, sel=100),
    "points/round1": _op("points", op_round_points, dict(strat=1, sel=100), needs=("list",), nobox=True, drops_point=True, strat=1, sel=100),
    # box
    "box/set1": _op("box", op_set_box, dict(seed=1), set_box=1),
    "box/set2": _op("box", op_set_box, dict(seed=2), set_box=2),
    "box/round2": _op("box", op_round_csr, dict(strat=2, sel=300), needs=LP + ("box",), strat=2, sel=300, anchor=True),
    "box/round4": _op("box", op_round_csr, dict(strat=4, sel=300), needs=LP + ("box",), strat=4, sel=300, anchor=True),
    "box/clear": _op("box", op_clear_box, needs=("box",), set_box=None),
    # dense
    "dense/round": _op("dense", op_dense_round, needs=("point",), pending_refused=True),
    "dense/round_gen": _op("dense", op_dense_round, dict(point="gen"), set_point="gen"),
    "dense/round_mid": _op("dense", op_dense_round, dict(point="mid"), set_point="mid"),
    "dense/eig": _op("dense", op_dense_eig, needs=("point",)),
    # tri: a complete adjacency, 4 T = 39 520 > every list but D
    "tri/prep": _op("tri", op_tri_prep, set_tri=True),
    "tri/sep10000": _op("tri", op_tri_separate, dict(max_out=10000), needs=("tri", "point")),
    "tri/sep0": _op("tri", op_tri_separate, dict(max_out=0), needs=("tri", "point")),
    # batch: explicit inputs, and the training set
    "batch/nn": _op("batch", op_nn_batch),
    "batch/eig": _op("batch", op_eig_batch),
    "batch/sdp": _op("batch", op_sdp_batch),
    "batch/data": _op("batch", op_train_data, set_train=True),
    "batch/loss_a": _op("batch", op_train_loss, dict(first=0, count=100), needs=("train",)),
    "batch/loss_b": _op("batch", op_train_loss, dict(first=100, count=157), needs=("train",)),
    # pool: stateful by design -- mirrored on a second long-lived handle, not on a fresh one
    "pool/create": _op("pool", op_pool_create, set_pool=True),
    "pool/add": _op("pool", op_pool_add, needs=("pool",)),
    "pool/step": _op("pool", op_pool_step, needs=("pool", "point")),
    "pool/step_gen": _op("pool", op_pool_step, dict(point="gen"), needs=("pool",), set_point="gen"),
    "pool/step_weak": _op("pool", op_pool_step, dict(point="weak"), needs=("pool",), set_point="weak"),
    "pool/state": _op("pool", op_pool_state, needs=("pool",)),
    "pool/destroy": _op("pool", op_pool_destroy, needs=("pool",), set_pool=False),
})
for _l in LISTS:
    OPS["list/" + _l] = _op("list", op_set_list, dict(name=_l), set_list=_l)
for _k, _names in NETS.items():
    for _n in _names:
        OPS["net/%d%s" % (_k, _n)] = _op("net", op_set_net, dict(k=_k, name=_n), set_net=(_k, _n))
for _o, (_id, _default, _values) in OPTIONS.items():
    for _v in _values:
        OPS["option/%s=%d" % (_o, _v)] = _op("option", op_set_option, dict(name=_o, value=_v), set_opt=(_o, _v),
                                             nobox=(_o == "exact_head" and _v == 1))


# ---- coverage ------------------------------------------------------------------------------------------------------------------------
def walk(tokens):
    """run a sequence through the model -> list of (index, name, family, marked refused, the model's verdict)"""
    m, out = Model(), []
    for i, tok in enumerate(tokens):
        marked, name = parse(tok)
        verdict = m.check(name)
        out.append((i, name, OPS[name]["fam"], marked, verdict))
        if verdict == "ok":
            m.apply(name)
    return out


def required_pairs():
    """-> (adjacent pairs, pairs with a `point` in between): every ordered pair of FAMILIES, and those with a round-like member"""
    direct = set(itertools.product(FAMILIES, FAMILIES))
    spaced = {(x, y) for x, y in direct if x in ROUND_LIKE or y in ROUND_LIKE}
    return direct, spaced


def covered_pairs(sequences):
    """-> (adjacent pairs, pairs with a `point` in between) that the sequences run.  An adjacent pair (X, Y) counts only where Y
    brings no LP point of its own -- such a Y clears the scored measures before it runs and IS the case with a point in between --
    or where X is a batched call, which has dropped the point anyway."""
    direct, spaced = set(), set()
    for tokens in sequences.values():
        ops = [OPS[parse(t)[1]] for t in tokens]
        fams = [op["fam"] for op in ops]
        for i in range(1, len(fams)):
            if "set_point" not in ops[i] or (ops[i - 1].get("drops_point") and not parse(tokens[i - 1])[0]):
                direct.add((fams[i - 1], fams[i]))
            if i >= 2 and fams[i - 1] == "point":
                spaced.add((fams[i - 2], fams[i]))
    return direct, spaced


# ---- the sequences -----------------------------------------------------------------------------------------------------------------
def _flips(setup, around):
    """every option to each of its other documented values and back to its default, `around` after every flip"""
    out = list(setup)
    for name in OPTIONS:
        _id, default, values = OPTIONS[name]
        for v in [v for v in values if v != default] + [default]:
            out += ["option/%s=%d" % (name, v)] + around
    return out


def _after(prefix, followers):
    return [t for f in followers for t in prefix + f]


_SKIPPED = ["point/strong", "round/csr4_5000"]      # on list C with skip = 2: the skipping and filtering launch, strong regime

HAND_SEQUENCES = {
    # tri_separate directly before and directly after a fused round: 4 T > N on A, B, C and E, not on D
    "HAND_tri_around_fused_rounds": ["tri/prep", "point/gen"] + _after([], [
        ["list/" + l, "tri/sep10000", "round/csr4", "tri/sep10000", "point/mid", "tri/sep0", "round/sel1", "tri/sep10000", "point/gen"]
        for l in "ABCED"]),
    # every entry visited (tie-aware sort), then count-rank selections with a head <= 8192 and of 9000
    "HAND_weak_round_then_count_rank": _after([], [
        ["list/" + l, "point/weak", "round/sel4_5000", "round/sel1_8192", "round/sel1_9000", "point/weak", "round/sel4_5000",
         "round/sel2_8192", "round/sel4_9000", "point/weak", "round/sel4_5000", "point/gen", "round/sel1_8192", "point/mid",
         "round/sel4_5000", "round/sel1_9000"] for l in "DC"]),
    # a skipped round in the strong regime, then at the same point everything that reads the measure it left partial
    "HAND_after_a_skipped_round": ["list/C", "option/skip=2", "option/exact_sdp=1"] + _after(_SKIPPED, [
        ["score/get"], ["rank/2"], ["score/sdp", "round/csr3"], ["multi/m5"], ["diverse/r4"], ["box/set1", "box/round4", "box/clear"],
        ["dense/round"], ["points/round4"], ["rank/1"], ["rows/cut"], ["round/sel2"], ["round/csr4_5000"], ["tri/prep", "tri/sep10000"],
        ["pool/create", "pool/add", "pool/step"], ["list/B", "round/csr4"]]),
    # a longer and a shorter list directly after a round (its epilogue has zeroed the spare selection workspace)
    "HAND_list_change_after_a_round": [
        "list/B", "point/gen", "round/csr4", "list/D", "round/csr4", "list/A", "round/csr4", "list/C", "round/sel1", "list/E", "round/sel2",
        "list/B", "round/csr1", "list/D", "round/sel4_5000", "list/A", "round/sel4", "list/D", "point/strong", "round/sel4_5000", "list/C",
        "round/sel4_5000", "list/B", "round/sel4_5000", "list/E", "round/csr4", "list/A", "points/round4", "list/D", "round/csrpt_weak",
        "list/B", "round/begin4", "round/end", "list/C", "round/begin1", "!score/eig", "!dense/round", "round/end", "list/A", "round/sel1"],
    # a view read completely, a call that needs a larger pinned block, a round again
    "HAND_view_then_a_larger_block": [
        "list/C", "point/gen", "round/view4", "round/csr4_5000", "round/view4", "multi/m5", "round/view4", "points/round4", "point/gen",
        "round/view4", "dense/round", "round/view4", "round/sel1_9000", "round/view4", "diverse/r4", "round/view4", "list/D",
        "round/view4", "rank/big", "round/view4"],
    # a ranking of more than 16 384 entries between two fused rounds
    "HAND_full_ranking_between_fused_rounds": [
        "list/D", "point/gen", "round/csr4", "rank/big", "point/gen", "round/csr4", "rank/big", "point/strong", "round/sel4_5000", "rank/big",
        "point/weak", "round/sel4_5000", "rank/big", "point/mid", "round/sel1_8192", "rank/big", "point/mid", "round/sel4_5000"],
    # option flips between two rounds at the same point, and ahead of a round that scores for itself
    "HAND_option_flips_same_point": _flips(["list/C", "point/strong", "round/csr4"], ["round/csr4"]),
    "HAND_option_flips_fresh_point": _flips(["list/E"], ["point/gen", "round/sel4"]),
    "HAND_option_flips_long_list": _flips(["list/D"], ["point/strong", "round/csr4_5000"]),
    # set_network between two rounds at the same point: the measure is recomputed, the filter margin changes with the tail networks
    "HAND_set_network_between_rounds": [
        "list/C", "option/skip=2", "point/strong", "round/csr4_5000", "net/3speaks", "round/csr4_5000", "net/3heard", "round/csr4",
        "net/3both", "round/csr4_5000", "net/3ship", "round/csr4_5000", "point/strong", "net/3both", "round/csr4_5000", "net/3ship",
        "list/E", "point/gen", "round/csr4", "net/4user", "round/csr4", "net/4ship", "round/csr4", "list/A", "round/sel2", "net/4user",
        "round/sel2", "net/4ship", "round/sel2", "batch/nn", "net/3heard", "batch/nn", "net/3ship", "batch/nn"],
    # reduced from HAND_option_flips_same_point, which failed at its round behind option/kernel=2: the optimality scores of the MFMA
    # kernel survived the change of variant and the round ranked them, where a fresh handle ranks the VALU kernel's (last bits).
    # sdpcut_set_option now invalidates them as sdpcut_set_network does (csrc/capi.hip)
    # a node box and SDPCUT_OPT_EXACT_HEAD refuse each other, whichever comes second; a round whose head plus band exceeds 8192
    # entries is refused while the option is on; the handle stays usable every time
    "HAND_box_and_exact_head_refuse_each_other": [
        "list/C", "point/strong", "box/set1", "!option/exact_head=1", "box/round4", "box/clear", "option/exact_head=1", "!box/set1",
        "round/csr4", "option/exact_head=0", "list/D", "option/exact_head=1", "!round/sel4_9000", "round/sel4_5000", "!round/sel2_8192",
        "round/sel1_9000", "!box/set2", "round/csr2", "option/exact_head=0", "round/sel4_9000", "box/set2", "!option/exact_head=1",
        "!points/round4", "box/round2", "box/clear", "points/round4"],
    "HAND_kernel_variant_change_scores_again": [
        "list/C", "point/strong", "round/csr4", "option/kernel=2", "round/csr4", "option/kernel=0", "round/csr4", "score/both",
        "option/kernel=2", "score/get", "rank/2", "option/kernel=2", "rank/2", "list/E", "score/nn", "option/kernel=0", "round/sel2"],
}

# Together: every ordered pair of FAMILIES adjacent, and every pair with a round-like member also with one `point` in between
# (test_op_sequences_cpu.py computes both from the lists).  PAIR_00 .. PAIR_07 were drawn once by a greedy seeded walk over the model
# that preferred variants not used yet and sent a box or a non-default option back after five operations; the script of that walk
# is not kept -- the lists are the data, and whoever changes the alphabet edits them by hand until the CPU test's set differences
# are empty again.  PAIR_08 is written by hand: the adjacent pairs the walk had covered only through a Y that brings its own LP
# point (which does not keep the scored measures of X alive, covered_pairs).
PAIR_SEQUENCES = {
    "PAIR_00": [
        "list/C", "point/psd", "points/round1", "box/set2", "batch/sdp", "!rows/all1", "list/B", "multi/m5pt_strong", "box/clear",
        "dense/eig", "option/fp32=0", "rows/all3", "net/3speaks", "diverse/r2pt_gen", "list/E", "option/fp32=1", "tri/prep",
        "multi/m1", "dense/round_mid", "box/set2", "score/nn", "multi/m1q50", "batch/eig", "net/4user", "box/clear", "rows/cut",
        "option/skip=2", "box/set2", "round/csrpt_strong", "batch/data", "!points/score", "option/skip=1", "diverse/r1",
        "box/clear", "net/3ship", "points/round4", "!rows/cut", "!score/both", "dense/round_gen", "batch/loss_a", "dense/eig",
        "dense/round", "diverse/filter", "score/both", "rows/all1", "rank/4", "batch/loss_b", "multi/m5sets", "diverse/filter",
        "rank/2", "score/eig", "batch/sdp", "rank/1", "list/E", "round/csr2", "net/3ship", "tri/prep", "rank/1", "dense/round",
        "rank/2", "rows/cut", "tri/sep0", "net/3speaks", "multi/m5sets", "net/3heard", "batch/loss_a", "tri/sep0", "dense/round",
        "multi/m1", "round/csrpt_gen", "dense/round", "list/B", "dense/round", "tri/sep0"
    ],
    "PAIR_01": [
        "list/E", "point/psd", "round/sel4_9000", "list/A", "box/set1", "box/round2", "multi/m1q50", "list/E", "rank/2",
        "box/clear", "option/fp32=1", "net/4user", "rank/1", "diverse/r2pt_gen", "option/fuse_keys=0", "option/fuse_keys=1",
        "score/eig", "list/A", "score/both", "tri/prep", "score/eig", "round/csr2", "pool/create", "multi/m5pt_strong", "score/sdp",
        "net/3ship", "pool/step_gen", "diverse/filter", "pool/step_weak", "option/one_launch=0", "points/round1", "batch/data",
        "batch/eig", "score/get", "option/one_launch=1", "list/A", "list/E", "net/3speaks", "net/4user", "round/csrpt_weak",
        "multi/m5pt_strong", "rows/all3", "dense/round_gen", "points/round4", "multi/m5pt_strong", "rank/2", "multi/m5pt_strong",
        "option/exact_head=0", "dense/round", "rows/cut", "rows/cut", "box/set1", "pool/destroy", "!points/round1", "tri/sep0",
        "diverse/r2pt_gen", "box/clear", "points/round4", "net/4user", "score/get", "diverse/r2pt_gen", "points/score",
        "pool/create", "box/set2", "!rank/3", "net/3ship", "list/C", "batch/eig", "box/clear", "list/D", "pool/state", "batch/data",
        "list/E", "tri/prep"
    ],
    "PAIR_02": [
        "list/D", "point/weak", "box/set1", "tri/prep", "round/view4", "tri/sep10000", "pool/create", "box/clear", "diverse/filter",
        "round/sel1_8192", "points/round1", "points/round1", "list/A", "!rows/all3", "points/score", "!rank/4", "points/score",
        "!score/eig", "!rank/4", "option/fuse_keys=1", "multi/m5pt_strong", "multi/m5pt_strong", "pool/step", "score/get",
        "score/get", "pool/step", "round/sel4", "score/nn", "points/round1", "diverse/r2pt_gen", "batch/sdp", "pool/destroy",
        "pool/create", "tri/prep", "tri/sep0", "list/E", "points/score", "round/csrpt_gen", "diverse/r2pt_gen", "multi/m1q50",
        "points/round4", "dense/round_gen", "score/both", "box/set2", "point/gen", "net/3heard", "rows/all1", "pool/destroy",
        "box/clear", "point/mid", "batch/eig", "round/sel4_9000", "option/fused_tail=0", "rank/1", "rank/4", "tri/sep10000",
        "option/skip=1", "option/fused_tail=1", "round/sel1", "round/view4", "rows/all1", "round/sel2", "box/set1", "point/psd",
        "rank/big", "round/sel4_9000", "rank/1", "box/clear", "point/weak", "round/sel1_9000", "point/gen", "option/fuse_keys=1",
        "pool/create", "rank/4"
    ],
    "PAIR_03": [
        "list/E", "point/strong", "multi/m1q50", "tri/prep", "batch/nn", "diverse/r1", "tri/sep10000", "box/set1", "point/strong",
        "!points/round4", "point/weak", "round/csr2", "box/clear", "point/strong", "tri/sep10000", "rows/all3", "batch/eig",
        "option/fuse_keys=1", "batch/nn", "point/weak", "dense/round_mid", "round/sel4_5000", "point/weak", "tri/sep0",
        "points/round1", "point/psd", "diverse/r4", "dense/round", "net/3speaks", "dense/eig", "pool/create", "rows/cut",
        "diverse/r4", "net/3both", "option/prefilter=0", "point/psd", "box/set2", "point/weak", "diverse/filter",
        "option/prefilter=1", "point/gen", "round/csrpt_strong", "box/clear", "point/weak", "box/set1", "point/psd", "rows/all1",
        "multi/m1q50", "point/psd", "box/clear", "point/mid", "list/D", "diverse/r1", "diverse/filter", "rows/all1", "point/mid",
        "dense/round", "point/psd", "multi/m1q50", "point/psd", "score/both", "point/weak", "points/round4", "point/weak",
        "box/set1", "point/gen", "dense/round_mid", "point/mid", "tri/sep0", "box/clear", "point/gen", "multi/m5pt_strong",
        "point/weak", "rank/big"
    ],
    "PAIR_04": [
        "list/B", "point/mid", "dense/round_mid", "point/weak", "round/sel4", "point/mid", "list/D", "point/psd", "diverse/filter",
        "point/weak", "rank/4", "pool/create", "list/A", "dense/eig", "point/mid", "dense/round_gen", "point/gen", "points/round4",
        "point/strong", "list/D", "net/4user", "point/psd", "points/round1", "point/mid", "rows/all1", "point/psd",
        "round/csrpt_gen", "point/gen", "rank/4", "point/mid", "multi/m5", "point/gen", "multi/m5sets", "point/strong",
        "dense/round_gen", "point/psd", "batch/nn", "point/gen", "multi/m1q50", "point/mid", "rows/cut", "point/weak", "box/set2",
        "point/gen", "score/eig", "point/psd", "box/set2", "box/clear", "point/psd", "option/fp32=1", "point/strong",
        "points/round1", "point/psd", "rank/2", "point/gen", "dense/eig", "point/weak", "option/fused_tail=1", "point/strong",
        "dense/eig", "point/gen", "diverse/filter", "point/weak", "tri/prep", "point/weak", "round/csr4", "point/mid",
        "dense/round", "point/weak", "list/B", "rows/all3", "point/gen", "points/round4", "point/mid"
    ],
    "PAIR_05": [
        "list/B", "point/strong", "option/one_launch=1", "point/mid", "multi/m1", "point/weak", "list/C", "score/eig", "point/weak",
        "dense/round_mid", "point/gen", "pool/create", "net/3speaks", "point/psd", "box/set2", "point/psd", "pool/create",
        "dense/round_gen", "point/psd", "box/clear", "multi/m5pt_strong", "point/psd", "batch/nn", "point/mid", "diverse/r1",
        "point/gen", "batch/eig", "point/psd", "box/set2", "option/kernel=2", "point/gen", "diverse/r4", "point/gen", "box/clear",
        "round/csr1", "option/kernel=0", "multi/m5sets", "point/mid", "pool/create", "point/psd", "dense/round", "point/weak",
        "score/get", "point/weak", "multi/m1q50", "point/strong", "points/score", "point/mid", "dense/round", "point/strong",
        "rows/all3", "point/mid", "multi/m5", "point/gen", "round/csrpt_weak", "point/mid", "diverse/r2pt_gen", "point/strong",
        "diverse/r2pt_gen", "point/gen", "points/score", "point/gen", "multi/m5sets", "point/psd", "option/one_launch=1", "rank/1",
        "point/gen", "points/score", "point/weak", "batch/sdp", "point/weak", "round/csrpt_gen", "point/psd", "score/sdp"
    ],
    "PAIR_06": [
        "list/A", "point/strong", "multi/m1", "point/gen", "net/3ship", "point/strong", "round/view4", "point/weak", "box/set2",
        "tri/prep", "point/psd", "box/round2", "score/nn", "box/clear", "diverse/filter", "point/weak", "round/csrpt_gen",
        "point/strong", "points/score", "point/mid", "option/exact_head=0", "multi/m1", "point/strong", "tri/sep10000", "point/gen",
        "points/round4", "point/weak", "pool/create", "point/mid", "diverse/r1", "point/strong", "pool/step_weak", "point/mid",
        "multi/m5", "point/gen", "diverse/filter", "point/strong", "score/eig", "point/psd", "round/sel2_8192", "point/mid",
        "net/3heard", "point/mid", "diverse/r2pt_gen", "point/strong", "rows/cut", "point/weak", "diverse/filter", "point/strong",
        "net/3both", "point/weak", "dense/round_mid", "point/psd", "rank/4", "point/psd", "diverse/r2pt_gen", "point/weak",
        "list/B", "dense/round_mid", "point/psd", "net/3heard", "point/psd", "multi/m5sets", "tri/sep10000", "point/psd",
        "diverse/r2pt_gen", "point/psd", "option/fuse_keys=1", "points/score", "point/mid", "net/3heard", "points/round4",
        "point/gen", "score/get"
    ],
    "PAIR_07": [
        "list/E", "point/mid", "tri/prep", "point/weak", "multi/m1", "tri/sep0", "point/mid", "dense/round_mid", "round/csr4",
        "point/weak", "batch/data", "point/strong", "points/score", "point/strong", "points/round4", "point/gen", "tri/sep10000",
        "diverse/filter", "point/gen", "multi/m5pt_strong", "score/eig", "point/weak", "diverse/r4", "point/psd", "dense/eig",
        "pool/create", "point/weak", "box/set2", "round/sel1", "point/mid", "multi/m5", "pool/step_gen", "box/clear", "rank/4",
        "point/gen", "round/sel1_9000", "point/strong", "round/csrpt_weak", "point/weak", "rows/all1", "round/csr4_5000",
        "point/gen", "pool/step_weak", "point/mid", "points/round4", "pool/step_weak", "point/psd", "round/sel4", "rank/2",
        "point/psd", "box/set2"
    ],
    "PAIR_08": [
        "list/C", "point/gen", "diverse/r1", "pool/create", "multi/m5", "dense/round", "pool/state", "dense/eig", "multi/m1",
        "multi/m5sets", "round/csr4", "diverse/r4", "round/sel2", "multi/m1q50", "list/B", "multi/m5", "net/3speaks", "diverse/r1",
        "net/3ship", "pool/add", "net/4user", "round/sel4", "rank/4", "diverse/filter", "rank/2", "multi/m5", "rows/cut",
        "dense/round", "score/both", "dense/eig", "point/strong", "score/eig", "diverse/r4", "net/4ship"
    ],
}

# Four seeded walks of 60 operations (their script is not kept either): a family at random, then a variant the model allows (one it refuses now and then)
RANDOM_SEQUENCES = {
    "RANDOM_0": [
        "list/D", "point/psd", "round/csr4", "dense/round", "round/csr4", "round/begin4", "!points/score", "!dense/round",
        "round/end", "round/csr4", "option/auto_regime=1", "round/csr2", "round/csr2", "dense/eig", "dense/round_gen", "tri/prep",
        "point/psd", "box/set2", "pool/create", "point/strong", "round/sel1", "tri/prep", "box/clear", "point/weak", "point/psd",
        "point/weak", "box/set2", "multi/m1", "round/csr4", "!points/round4", "batch/nn", "box/clear", "round/csr4", "points/score",
        "round/csrpt_gen", "net/3ship", "round/csr2", "round/sel2", "box/set1", "net/3heard", "diverse/filter", "round/view4",
        "net/4ship", "box/clear", "points/round1", "point/gen", "round/csrpt_gen", "round/sel4_9000", "batch/sdp", "multi/m1",
        "list/D", "tri/sep0", "rank/big", "net/4user", "option/prefilter=0", "points/score", "option/count_rank=1",
        "multi/m5pt_strong", "rank/2", "option/prefilter=1"
    ],
    "RANDOM_1": [
        "list/B", "point/psd", "net/3heard", "box/set2", "!points/round1", "option/prefilter=1", "rank/big", "point/psd",
        "box/clear", "rank/2", "option/prefilter=1", "round/sel4_9000", "tri/prep", "points/round4", "!rank/1", "diverse/r2pt_gen",
        "point/psd", "list/C", "dense/eig", "point/weak", "rank/big", "point/weak", "option/prefilter=1", "option/fused_tail=0",
        "rows/cut", "list/B", "tri/prep", "score/sdp", "option/fused_tail=1", "box/set2", "!points/round1", "net/3heard",
        "score/eig", "dense/eig", "box/clear", "round/begin4", "round/end", "rank/1", "diverse/r1", "rows/all3", "round/csr4_5000",
        "round/csr2", "tri/sep0", "multi/m1q50", "round/begin4", "round/end", "option/count_rank=0", "points/round4", "point/weak",
        "list/E", "multi/m1", "option/count_rank=1", "points/score", "dense/round_mid", "option/skip=1", "tri/sep10000",
        "net/3ship", "round/begin1", "round/end", "pool/create"
    ],
    "RANDOM_2": [
        "list/C", "point/gen", "batch/sdp", "multi/m5", "list/C", "point/weak", "rank/1", "dense/round_gen", "round/csr4",
        "net/4user", "round/sel4", "round/view4", "list/A", "point/gen", "list/C", "point/gen", "multi/m5sets", "round/begin1",
        "!dense/round", "!score/eig", "round/end", "pool/create", "multi/m1q50", "net/4user", "rank/1", "diverse/filter",
        "batch/sdp", "points/round1", "list/D", "batch/data", "round/csrpt_strong", "point/weak", "point/gen", "option/fuse_keys=1",
        "rows/cut", "diverse/filter", "list/B", "points/round4", "round/csrpt_gen", "point/weak", "list/B", "point/strong",
        "round/view4", "dense/round_mid", "pool/step_weak", "list/D", "rank/2", "rank/2", "points/score", "!rows/all1",
        "!rows/all1", "multi/m5pt_strong", "score/get", "multi/m5", "box/set1", "dense/round_gen", "score/both",
        "option/count_rank=1", "rows/all1", "box/clear"
    ],
    "RANDOM_3": [
        "list/C", "point/strong", "rank/1", "batch/data", "points/score", "pool/create", "list/A", "tri/prep", "!score/both",
        "score/get", "point/strong", "option/count_rank=0", "option/exact_sdp=0", "batch/eig", "tri/sep0", "points/score",
        "option/count_rank=1", "!score/eig", "list/A", "round/csrpt_gen", "dense/round_gen", "point/weak", "points/score",
        "!score/sdp", "round/csrpt_gen", "box/set2", "rank/1", "net/3ship", "rows/all3", "multi/m5", "box/clear", "round/sel1",
        "rank/4", "diverse/r1", "diverse/r1", "score/eig", "pool/step_gen", "list/A", "list/E", "box/set1", "list/A", "box/round4",
        "round/csr2", "point/gen", "box/clear", "round/sel4", "pool/create", "batch/loss_b", "option/kernel=2", "dense/round",
        "dense/round_mid", "round/sel1_8192", "diverse/filter", "option/kernel=0", "tri/prep", "rows/all1", "round/sel1_9000",
        "points/score", "multi/m5pt_strong", "dense/round"
    ],
}

SEQUENCES = {}
for _group in (PAIR_SEQUENCES, HAND_SEQUENCES, RANDOM_SEQUENCES):
    SEQUENCES.update(_group)


