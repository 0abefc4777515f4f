"""Host-side mirror of the reference's cut-selection surface, backed by the GPU library.

The cutting-plane loop of the reference (cut_select_qp.py:149-200, cut_select_qcqp.py:63-112)
talks to the hot path through four methods of ``CutSolver``:

    _load_neural_nets()                                               cut_select_qp.py:284-303
    _sel_eigcut_by_ordering_on_measure(strat, vars_values, cut_round, sel_size=0)   :543-703
    _gen_eigcuts_selected(strat, sel_size, rank_list, strong_only=False, vars_values=None)  :705-755
    _get_eigendecomp(dim_subpr, curr_pt, X_slice, ev_yes)             :788-797

:class:`GpuCutSelectionMixin` provides exactly these, with the same arguments, return layouts
and ordering, reading the same instance state (``self._agg_list``, ``self._nb_lifted``,
``self._Q_arr``, ``self._nb_vars``, ``self._dim``, ``self._my_prob``).  Put it in front of the
reference class to drop it into the unmodified loop:

    class GpuCutSolver(GpuCutSelectionMixin, cut_select_qp.CutSolver): pass

All arithmetic (gather, eigen-decomposition, MLP, ranking, cut coefficients) runs in
libsdpcut_hip.so; this file only marshals arrays and builds the Python objects the loop
expects.  No CPU fallback exists: without the library / a gfx950 GPU the methods raise.
"""
from types import SimpleNamespace

import numpy as np

from . import _capi, networks
from .rank_list import (AggArrays, DeviceAgg, FeasEntry, RankList, RankListHead, _BIG_M, _Binding, _Concat,  # noqa: F401
                        csr_prefix, rows_to_csr, strong_prefix)

_THRES_NEG_EIGVAL = -10 ** (-15)      # cut_select_qp.py:24
_HEAD = 5000                          # _SDP_CUTS_PER_ROUND_MAX (:37): rank-list head fetched eagerly
_FUSED_HEAD_MAX = 16384               # longest head the fused round (sdpcut_round_csr) assembles
# what each selecting strategy has the device score: feasibility, optimality (MLP), exact optimality, combined, efficacy (which
# scores lambda_min with it)
_MEASURES = {1: _capi.EIG, 2: _capi.NN, 3: _capi.SDP, 4: _capi.EIG | _capi.NN, 6: _capi.EIG | _capi.EFF}
_OPT_STRATS = (2, 3, 4, -1, 6)        # strategies whose rank-list entries are optimality tuples (cut_select_qp.py:599); 6 ranks as 2 does
_STRONG_STRATS = (2, 3, 4, -1)        # ... and for which strong_only cuts the head at the first non-positive score (:725-726)


def _lp_point(vars_values):
    """the LP point as a contiguous float64 array: the caller's own array where it already is one"""
    if isinstance(vars_values, np.ndarray) and vars_values.dtype == np.float64 and vars_values.flags.c_contiguous:
        return vars_values
    return np.ascontiguousarray(vars_values, dtype=np.float64)


_SPARSE_PAIR = None


def _default_sparse_pair():
    """cplex.SparsePair if the reference's LP library is installed, else the stand-alone twin; looked up once
    (a failing ``import cplex`` walks the whole module path: ~60 us per call, once per round before it was cached)"""
    global _SPARSE_PAIR
    if _SPARSE_PAIR is None:
        try:
            import cplex                      # the reference's LP object, if installed
            _SPARSE_PAIR = cplex.SparsePair
        except ImportError:
            from .harness import SparsePair
            _SPARSE_PAIR = SparsePair
    return _SPARSE_PAIR


class GpuCutSelectionMixin(object):
    """The four hot-path methods of the reference's ``CutSolver`` on the GPU."""

    _gpu_device = 0
    _sparse_pair = None
    _gpu_overlap = True      # begin the follower list's round together with the leader's (QCQP: two covers per LP point)
    # heads under the NN-ranked strategies (2, 4) ordered and reported by obj_improve in the reference's operation order
    # (SDPCUT_OPT_EXACT_HEAD, include/sdpcut.h); a subclass or make_dropin_classes(..., exact_heads=True) switches it on
    _gpu_exact_heads = False
    # strategies 3 (optimality via the exact SDP solution) and -1 (figure 8: estimated against exact measure) on the device
    # (SDPCUT_OPT_EXACT_SDP, SDPCUT_SDP; exact_sdp.py is the numpy twin of the solver); off: both are refused as before
    _gpu_exact_sdp = False
    # all violated eigen-cuts of a selected set: with cuts_per_set > 1 _gen_eigcuts_selected emits up to
    # that many rows per selected set (Scorer.cut_rows_all) and keeps the first quota of them in list order -- the sel_size it is
    # called with, or cuts_per_set times that with cuts_row_quota = "sets".  make_dropin_classes(..., cuts_per_set=m) sets it.
    cuts_per_set = 1
    cuts_row_quota = None
    # the variable bounds of the branch-and-bound node the solver works at (set_node_box): None = the root's unit box
    _gpu_node_box = None

    # ------------------------------------------------------------------ a11 loader
    def _load_neural_nets(self):
        """Create the GPU handle pool and upload the MLPs for d = 2..self._dim
        (replaces the ctypes load of NNs.so, cut_select_qp.py:284-303)."""
        self._gpu_nets = {}
        for d in range(2, self._dim + 1):
            self._gpu_nets[d] = networks.load_network(d)
        # one entry per dimension like the reference's (func, buffer) list, for code that
        # only checks its length
        self._nns = [(None, None)] * (self._dim - 1)
        self._gpu_bindings = {}

    def _gpu_wake(self):
        """Poke the device(s) of the bound candidate lists (sdpcut_wake): called the moment an LP solve returns, while the solution
        vector is still being extracted -- a round issued to a device that idled through the solve costs 0.1-0.2 ms more than one
        issued back to back, and this gets 40-65 us of it back (bench.py: secondary.cold_round).  A maintainer of the reference's
        own loop adds `self._gpu_wake()` behind `my_prob.solve()` (cut_select_qp.py:194); optional, changes no result."""
        for b in getattr(self, "_gpu_bindings", {}).values():
            b.scorer.wake()

    # ------------------------------------------------------------------ device binding
    def _gpu_new_scorer(self):
        sc = _capi.Scorer(self._gpu_device)
        for d, (widths, params) in getattr(self, "_gpu_nets", {}).items():
            sc.set_network(d, widths, params)
        if self._gpu_exact_heads:
            sc.set_option(_capi.OPT_EXACT_HEAD, 1)
        if self._gpu_exact_sdp:
            sc.set_option(_capi.OPT_EXACT_SDP, 1)
        return sc

    def _gpu_bind(self):
        """Scorer bound to the current ``self._agg_list`` (cached per list object: the QCQP
        loop swaps two lists every round, cut_select_qcqp.py:75-78)."""
        if not hasattr(self, "_gpu_bindings") or self._gpu_bindings is None:
            self._gpu_bindings = {}
        if not hasattr(self, "_gpu_nets"):
            self._gpu_nets = {}
        agg = self._agg_list
        key = id(agg)
        b = self._gpu_bindings.get(key)
        if b is not None and b.agg_list is agg and b.n_at_bind == len(agg) and b.serial == getattr(agg, "serial", 0):
            return b
        N = len(agg)
        if isinstance(agg, DeviceAgg):          # the list already lives on its scorer
            b = _Binding(agg.scorer, agg, self._nb_vars, self._nb_lifted)
            b.n_at_bind, b.serial = N, agg.serial
            self._gpu_bindings[key] = b
            return b
        if isinstance(agg, AggArrays):          # enumerated on our side: the arrays already exist
            S, ks = agg.set_inds, agg.ks
        else:
            S = np.full((max(N, 1), 5), -1, dtype=np.int32)
            ks = np.zeros(max(N, 1), dtype=np.int32)
            for i, e in enumerate(agg):
                s = e[0]
                ks[i] = len(s)
                S[i, :len(s)] = s
        sc = self._gpu_new_scorer()
        sc.set_instance(self._nb_vars, np.asarray(self._Q_arr, dtype=np.float64))
        sc.set_candidates(S[:N], ks[:N])
        if self._gpu_node_box is not None:
            sc.set_box(*self._gpu_node_box)
        b = _Binding(sc, agg, self._nb_vars, self._nb_lifted)
        b.n_at_bind = N
        b.ks, b.set_arr = ks[:N], S[:N]
        b.serial = getattr(agg, "serial", 0)
        self._gpu_bindings[key] = b
        return b

    def gpu_bind_arrays(self, set_inds, ks, nb_vars, Q_arr, global_base=0):
        """Array entry (no Python agg_list): used for large synthetic / enumerated covers."""
        if not hasattr(self, "_gpu_nets"):
            self._gpu_nets = {}
        sc = self._gpu_new_scorer()
        sc.set_instance(nb_vars, Q_arr)
        sc.set_candidates(set_inds, ks, global_base)
        if self._gpu_node_box is not None:
            sc.set_box(*self._gpu_node_box)
        b = _Binding(sc, None, nb_vars, nb_vars * (nb_vars + 1) // 2)
        b.set_arr, b.ks, b.n_at_bind = np.asarray(set_inds), np.asarray(ks), len(ks)
        return b

    def set_node_box(self, lb, ub):
        """The solver works at a branch-and-bound node with the variable bounds ``lb <= x <= ub`` (both None: back at the root):
        every handle bound to the solver, and every one it creates later (:meth:`_gpu_bind` for a host-side list,
        :meth:`gpu_bind_arrays`), computes the optimality measures of strategies 2, 3 and 4 for the node's small SDP
        (``Scorer.set_box``, :mod:`nodebox`); eigenvalues, the violated test and the cuts do not depend on bounds.  A list that
        lives on a scorer of its own (``DeviceAgg``) and is bound AFTER this call keeps whatever box that scorer has: set it
        there, or call this method again once the list is bound.  ``cut_select_algo`` takes its box as an argument and neither
        uses nor changes this one.  The caller's LP carries the node's bounds itself (``harness.boxqp_relaxation(inst, lb, ub)``)."""
        self._gpu_node_box = box = self._gpu_check_box(lb, ub)
        for b in (getattr(self, "_gpu_bindings", None) or {}).values():
            self._gpu_apply_box(b, box)

    def _gpu_check_box(self, lb, ub):
        """(lb, ub) as checked [n] arrays (scalars are broadcast), or None for no box"""
        if lb is None and ub is None:
            return None
        from .nodebox import check_box
        n = self._nb_vars
        return check_box(n, np.broadcast_to(np.asarray(lb, dtype=np.float64), (n,)), np.broadcast_to(np.asarray(ub, dtype=np.float64), (n,)))

    @staticmethod
    def _gpu_apply_box(b, box):
        b.drain()
        if box is None:
            b.scorer.clear_box()
        else:
            b.scorer.set_box(*box)
        b.scored &= _capi.EIG      # (the library keeps lambda_min and drops the measures of the old box)
        b.rank_serial += 1

    @staticmethod
    def _gpu_point(b, vars_values, flags):
        """Make ``vars_values`` the device's LP point and score what ``flags`` asks for.

        The upload is skipped only when the point equals -- entry by entry -- the copy kept of the last one
        uploaded through this binding (an in-place edit of the caller's array is a new point); the upload
        itself is an asynchronous copy out of pinned staging, so a redundant one costs little.
        :meth:`invalidate_point` forces the next call to upload."""
        b.drain()
        vv = _lp_point(vars_values)
        same = b.point_copy is not None and b.point_copy.shape == vv.shape and np.array_equal(vv, b.point_copy)
        if not same:
            b.scorer.set_point(vv)
            b.note_point(vv)
        need = flags & ~b.scored
        if need:
            b.scorer.score(need)
            b.scored |= need
        return vv

    def invalidate_point(self):
        """Forget which LP point the device holds: the next selection / generation uploads its point whatever it is
        (for callers that change device state behind the mixin's back, e.g. through the Scorer directly)."""
        for b in getattr(self, "_gpu_bindings", {}).values():
            b.drain()
            b.point_copy, b.scored = None, 0

    # ------------------------------------------------------------------ a7-a9 selection
    def _sel_eigcut_by_ordering_on_measure(self, strat, vars_values, cut_round, sel_size=0):
        """Strategies 1 (feasibility), 2 (optimality via MLP), 4 (combined), 5 (random); same returns as
        cut_select_qp.py:543-703.  Strategy 6 (efficacy of the emitted row, ``Scorer.score(EFF)``; not the reference's) returns
        the layout of strategy 2 with the efficacy score in place of obj_improve.  With ``_gpu_exact_sdp`` also 3 (optimality via the exact SDP solution: the layout of strategy 2)
        and -1 (figure 8: ``(rank_list, overlap, std_dev_exact, this_round_cuts)`` of :660-702)."""
        if strat == 5:
            # random order, in place, like :634-637; the device twin of the old order is dropped
            agg = self._agg_list
            if isinstance(agg, DeviceAgg):
                agg = self._agg_list = agg.to_arrays()
            if isinstance(agg, AggArrays):
                agg.shuffle()
            else:
                np.random.shuffle(agg)
            getattr(self, "_gpu_bindings", {}).pop(id(agg), None)
            return agg
        if strat not in (1, 2, 4, 6) and not (self._gpu_exact_sdp and strat in (3, -1)):
            raise NotImplementedError("exact-SDP strategies (3, -1) are not part of the GPU path unless exact_sdp is switched on")
        b = self._gpu_bind()
        N = len(self._agg_list)
        sel_size = min(sel_size, N)
        if strat == -1:
            return self._gpu_figure8(b, vars_values, cut_round, sel_size)
        flags = _MEASURES[strat]
        if N == 0:
            return []       # strat 4 included: sel_size is clamped to 0 and the reference falls through
        # head fetched eagerly: what the loop can consume (sel_size is only passed for strat 4;
        # for 1 / 2 the cap of :37 bounds it)
        head = min(N, sel_size if (strat == 4 and sel_size > 0) else _HEAD)
        vv = _lp_point(vars_values)
        fused = None
        # which list is ranked by feasibility right after which at the same point: the QCQP loop's pair (cut_select_qcqp.py:64-76)
        last = getattr(self, "_gpu_last", None)
        if (self._gpu_overlap and strat == 1 and last is not None and last[0] is not b and last[0].follower is None
                and last[0].leader is None and b.follower is None and b.leader is None and 1 <= head <= _FUSED_HEAD_MAX and last[1].shape == vv.shape and np.array_equal(last[1], vv)):
            last[0].follower, b.leader = (b, head), last[0]
        if 1 <= head <= _FUSED_HEAD_MAX and not (strat == 4 and sel_size == 0):
            # ONE library call for the whole separation step (cut_select_qp.py:165-182): LP point up, scores, ranking
            # AND the assembled cuts of the head, which _gen_eigcuts_selected then only hands to the LP.  In two halves:
            # between them the follower list's round is begun too, so both covers' device work overlaps.
            pend = b.pending
            if pend is not None and not (pend[0] == strat and pend[1] == head and pend[2].shape == vv.shape and np.array_equal(pend[2], vv)):
                b.drain()
                pend = None
            f = b.follower
            spec = f is not None and f[0].pending is None and f[0] is not b
            if spec and b.n_at_bind < f[0].n_at_bind:
                # the longer list's round is begun first; the shorter one's few small kernels go ahead of its waiting
                # workgroups on a high-priority stream (SDPCUT_OPT_STREAM_PRIORITY), so this call still returns early
                if not b.prioritised:
                    b.drain()
                    b.scorer.set_option(_capi.OPT_STREAM_PRIORITY, 1)
                    b.prioritised, pend = True, None
                f[0].begin(1, f[1], vv, _capi.EIG)
                spec = False
            if pend is None:
                b.begin(strat, head, vv, flags)
            if spec:
                if f[0].n_at_bind < b.n_at_bind and not f[0].prioritised:      # (the other way round: the follower is the short list)
                    f[0].scorer.set_option(_capi.OPT_STREAM_PRIORITY, 1)
                    f[0].prioritised = True
                f[0].begin(1, f[1], vv, _capi.EIG)
            fused = b.end()
            idx, score = fused["idx"].copy(), fused["score"].copy()
            total, new_strat, counters = fused["n_total"], fused["new_strat"], fused["counters"]
            self._gpu_last = (b, b.point_copy)
        else:
            self._gpu_last = None
            vv = self._gpu_point(b, vv, flags)
            idx, score, total, new_strat, counters = b.scorer.rank(strat, sel_size, head)
        b.rank_serial += 1
        rl = RankList(b, 1 if strat == 1 else 2, total, vv, idx, score, strat=strat, sel_size=sel_size, fused=fused)
        rl.counters = counters
        if strat == 4:
            # the reference divides by sel_size and swallows the ZeroDivisionError, falling
            # through to `return rank_list` (cut_select_qp.py:629-632, 703)
            return rl if sel_size == 0 else (new_strat, rl)
        return rl

    def _gpu_figure8(self, b, vars_values, cut_round, sel_size):
        """Strategy -1 (cut_select_qp.py:660-702): both measures of every candidate from the device -- the MLP's estimate and the
        exact SDP optimum, ``p* max_elem - S max_elem`` -- and the reference's comparison of the two orderings in numpy
        (exact_sdp.figure8).  -> (rank_list by the estimated measure, overlap / sel_size, std_dev_exact, this_round_cuts)."""
        from . import exact_sdp
        vv = self._gpu_point(b, vars_values, _capi.NN | _capi.SDP)
        self._gpu_last = None
        _, nn = b.scorer.get_scores(eig=False)
        exact, _ = b.scorer.get_sdp_scores()
        order, overlap, std_dev_exact, rows = exact_sdp.figure8(nn, exact, cut_round, sel_size)
        b.rank_serial += 1
        # the whole list is on the host already: the rank list never goes back to the device (strategy 2's order, :688)
        rl = RankList(b, 2, nn.shape[0], vv, order + b.scorer.base, nn[order], strat=2, sel_size=sel_size)
        return rl, overlap, std_dev_exact, rows

    # ------------------------------------------------------------------ a10 generation
    def _gpu_pair(self):
        """the per-row object of a reference-style row store: ``self._sparse_pair``, else the installed LP library's"""
        return self._sparse_pair or _default_sparse_pair()

    def _gpu_add_csr(self, csr, pair=None, copy=True, integral=False):
        """Hand a block of assembled cuts ``(indptr, indices, values, rhs)`` to the LP; the one place that knows the two kinds of
        row store: as arrays when the store takes them (``add_csr``), else as the reference's per-row objects
        (cut_select_qp.py:747-754) with Python int indices and float values.  ``csr=None`` hands over nothing, the way the
        reference adds its empty lists.  copy: the arrays are views of a scorer's pinned block, which the next round overwrites, so
        the store gets copies; a caller that built the arrays itself passes False.  integral: the per-row objects carry integer
        coefficients and right-hand sides (the triangle rows, :833-836).  -> number of rows."""
        store = self._my_prob.linear_constraints
        if csr is None:
            store.add(lin_expr=[], rhs=[], senses=[])
            return 0
        indptr, ind, val, rhs = csr
        r = rhs.shape[0]
        if hasattr(store, "add_csr"):
            if copy:
                indptr, ind, val, rhs = np.array(indptr), np.array(ind), np.array(val), np.array(rhs)      # (int32 index arrays as the device wrote them)
            store.add_csr(indptr, ind, val, rhs, "G")
            return r
        pair = pair or self._gpu_pair()
        ptr, ind, val, rhs = indptr.tolist(), ind.tolist(), val.tolist(), rhs.tolist()
        if integral:
            val, rhs = [int(v) for v in val], [int(v) for v in rhs]
        store.add(lin_expr=[pair(ind=ind[ptr[c]:ptr[c + 1]], val=val[ptr[c]:ptr[c + 1]]) for c in range(r)], rhs=rhs, senses=["G"] * r)
        return r

    def _rank_groups(self, strat, sel_size, rank_list, strong_only):
        """The first ``sel_size`` entries of a rank list as runs of (binding, global candidate ids) in list order, or None where an
        entry cannot be traced to a bound candidate.  The one walk from what the loop hands to cut generation -- a RankList, its
        head, a concatenation of such (cut_select_qcqp.py:79), the shuffled list of strategy 5, plain entry lists -- to what the
        device can be asked about."""
        opt_sel = strat in _OPT_STRATS

        def of_rank_list(rl, count, cut_at_nonpositive):
            idx = np.asarray(rl.ids(count), dtype=np.int64)
            if cut_at_nonpositive:                            # cut_select_qp.py:725-726
                idx = idx[:strong_prefix(rl.scores(count), count)]
            return rl._b, idx

        def of_entries(entries, as_opt):
            if as_opt:
                if strong_only:
                    cut = next((p for p, e in enumerate(entries) if e[1] <= 0), len(entries))
                    entries = entries[:cut]
                return [(self._gpu_bind(), np.array([e[0] for e in entries], dtype=np.int64))]
            if not all(isinstance(e, FeasEntry) and e.binding is not None for e in entries):
                return None
            # runs of entries of one candidate list (the QCQP feasibility round concatenates the lists of two covers)
            runs = []
            for e in entries:
                if runs and runs[-1][0] is e.binding:
                    runs[-1][1].append(e.agg_idx)
                else:
                    runs.append((e.binding, [e.agg_idx]))
            return [(g, np.array(ix, dtype=np.int64)) for g, ix in runs]

        if isinstance(rank_list, _Concat):
            groups, left = [], sel_size
            for part in rank_list._parts:
                if left <= 0:
                    break
                take = min(left, len(part))
                rl = part.parent if isinstance(part, RankListHead) else part
                if isinstance(rl, RankList):
                    groups.append(of_rank_list(rl, take, opt_sel and strong_only and rl._kind != 1))
                else:
                    entries = list(part[0:take])
                    g = of_entries(entries, bool(entries) and not isinstance(entries[0], FeasEntry) and opt_sel)
                    if g is None:
                        return None
                    groups.extend(g)
                left -= take
            return groups
        if isinstance(rank_list, RankListHead):
            rank_list, sel_size = rank_list.parent, min(sel_size, len(rank_list))
        if isinstance(rank_list, RankList):
            return [of_rank_list(rank_list, sel_size, opt_sel and strong_only)]
        if strat == 5 and rank_list is self._agg_list:
            # random selection (:729-732): the shuffled list itself, entries 0 .. sel_size-1
            b = self._gpu_bind()
            return [(b, np.arange(min(sel_size, len(rank_list)), dtype=np.int64) + b.scorer.base)]
        return of_entries(list(rank_list[0:sel_size]), opt_sel)

    def _fused_blocks(self, strat, sel_size, rank_list, strong_only, vars_values):
        """The cuts of the first ``sel_size`` entries as the blocks their fused rounds assembled, in list order: one of a rank
        list or its head, one per part of ``(A + B)[0:sel_size]`` of the QCQP round; None unless every part still has them."""
        mixed = isinstance(rank_list, _Concat)
        blocks, left = [], sel_size
        for part in (rank_list._parts if mixed else [rank_list]):
            if left <= 0:
                break
            take = min(left, len(part))
            rl = part.parent if isinstance(part, RankListHead) else part
            if not isinstance(rl, RankList):
                return None
            feas = rl._kind == 1 if mixed else strat == 1
            csr = rl.fused_rows(take, strong_only=strong_only and strat in _OPT_STRATS and not feas, vars_values=vars_values if feas else None)
            if csr is None:
                return None
            blocks.append(csr)
            left -= take
        return blocks

    def _gen_eigcuts_selected(self, strat, sel_size, rank_list, strong_only=False, vars_values=None):
        """Eigen-cuts of the first ``sel_size`` ranked candidates, appended to
        ``self._my_prob.linear_constraints`` (cut_select_qp.py:705-755).  ``strong_only`` has no meaning under strategy 6 (a
        non-positive score there is a candidate that yields no cut anyway) and is ignored."""
        strong_only = strong_only and strat in _STRONG_STRATS
        if int(self.cuts_per_set) > 1 and sel_size > 0 and len(rank_list) > 0:
            return self._gen_eigcuts_multi(strat, sel_size, rank_list, strong_only, vars_values)
        sel_size = min(sel_size, len(rank_list))
        if sel_size <= 0:
            return self._gpu_add_csr(None)
        # the rows the fused round assembled, if its block still has them
        blocks = self._fused_blocks(strat, sel_size, rank_list, strong_only, vars_values)
        if blocks is not None:
            return sum(self._gpu_add_csr(c) for c in blocks)
        # else the candidates' rows from the device, else (entries that name no bound candidate) the generic path
        groups = self._rank_groups(strat, sel_size, rank_list, strong_only)
        if groups is None:
            return self._gen_from_entries(list(rank_list[0:sel_size]), strat == 1, vars_values, self._gpu_pair())
        # optimality cuts at the point the list was ranked at, feasibility cuts at the caller's
        rl = rank_list.parent if isinstance(rank_list, RankListHead) else rank_list
        vv = rl._vv if strat in _OPT_STRATS and isinstance(rl, RankList) else None
        if vv is None:
            vv = vars_values
        parts = []
        for g, idx in groups:
            if idx.size:
                self._gpu_point(g, vv, 0)
                parts.append(g.scorer.cut_rows(idx - g.scorer.base))
        if not parts:
            return self._gpu_add_csr(None)
        lam, coef, rhs, cols, ks = (np.concatenate(a) for a in zip(*parts)) if len(parts) > 1 else parts[0]
        keep = np.nonzero(lam < _THRES_NEG_EIGVAL)[0]          # :743
        # batched assembly (SURVEY 8 f row 4): the padded device rows become one CSR block with
        # array operations, no Python object per cut
        return self._gpu_add_csr(rows_to_csr(coef[keep], cols[keep], ks[keep]) + (rhs[keep],), copy=False)

    # ------------------------------------------------------------------ all violated eigen-cuts of a selected set
    def _multi_log_add(self, **rec):
        if getattr(self, "multi_log", None) is None:
            self.multi_log = []
        self.multi_log.append(rec)

    def _gen_eigcuts_multi(self, strat, sel_size, rank_list, strong_only, vars_values):
        """_gen_eigcuts_selected with ``cuts_per_set`` > 1: every selected set offers up to that many eigen-cuts
        (``Scorer.cut_rows_all``: one decomposition per set on the device), the first ``sel_size`` rows in list order are kept
        (``cuts_row_quota = "sets"``: the first ``cuts_per_set * sel_size``).  One record per call goes to ``self.multi_log``."""
        m = int(self.cuts_per_set)
        quota = int(sel_size) * (m if self.cuts_row_quota == "sets" else 1)
        groups = self._rank_groups(strat, min(sel_size, len(rank_list)), rank_list, strong_only)
        if groups is None:
            raise NotImplementedError("cuts_per_set > 1 needs rank lists whose entries name candidates bound to the device")
        vv = vars_values
        if vv is None:
            rl = rank_list.parent if isinstance(rank_list, RankListHead) else rank_list
            vv = getattr(rl, "_vv", None)
        coef, rhs, cols, ks, per_entry = [], [], [], [], []
        for g, idx in groups:
            if idx.size:
                self._gpu_point(g, vv, 0)
                rp, _, co, rh, cl, kk = g.scorer.cut_rows_all(idx - g.scorer.base, m)
                n = np.diff(rp)
                ent = np.repeat(np.arange(idx.shape[0]), n)
                coef.append(co), rhs.append(rh), cols.append(cl[ent]), ks.append(kk[ent]), per_entry.append(n)
        if not coef:
            self._multi_log_add(strat=strat, entries=0, entries_used=0, rows=0, offered=0, offered_hist=[0] * (m + 1), quota=quota, quota_hit=False)
            return self._gpu_add_csr(None)
        coef, rhs, cols, ks, per_entry = (np.concatenate(a) for a in (coef, rhs, cols, ks, per_entry))
        offered = int(coef.shape[0])
        rows = min(offered, quota)
        starts = np.concatenate([[0], np.cumsum(per_entry)[:-1]])
        self._multi_log_add(strat=strat, entries=int(per_entry.shape[0]), entries_used=int(np.count_nonzero((per_entry > 0) & (starts < rows))),
                            rows=rows, offered=offered, offered_hist=np.bincount(per_entry, minlength=m + 1).tolist(), quota=quota,
                            quota_hit=offered > quota)
        return self._gpu_add_csr(rows_to_csr(coef[:rows], cols[:rows], ks[:rows]) + (rhs[:rows],), copy=False)

    # ------------------------------------------------------------------ dense eigen-cuts (strategy 0)
    def _gpu_dense_scorer(self):
        """Handle that holds the instance for the dense eigen-cuts (no candidates, no networks): made once per instance."""
        key = (self._nb_vars, id(self._Q_arr))
        if getattr(self, "_gpu_dense_key", None) != key:
            sc = _capi.Scorer(self._gpu_device)
            sc.set_instance(self._nb_vars, np.asarray(self._Q_arr, dtype=np.float64))
            self._gpu_dense_sc, self._gpu_dense_key = sc, key
        return self._gpu_dense_sc

    def _gen_dense_eigcuts(self, vars_values=None):
        """One fully dense eigen-cut per negative eigenvalue (but the largest) of the whole lifted matrix at ``vars_values``,
        appended to the LP (cut_select_qp.py:757-786); decomposition and rows on the device (sdpcut_dense_round).
        -> number of cuts."""
        r = self._gpu_dense_scorer().dense_round(_lp_point(vars_values))
        nb, cols = r["n_rows"], r["cols"]
        # (values and rhs are copied: they are views of the scorer's pinned block, which the next round overwrites)
        return self._gpu_add_csr((np.arange(nb + 1, dtype=np.int64) * cols.shape[0], np.tile(cols, nb), r["values"].reshape(-1).copy(),
                                  r["rhs"].copy()), copy=False)

    # the reference's loop reaches it through the name-mangled private name (cut_select_qp.py:166)
    _CutSolver__gen_dense_eigcuts = _gen_dense_eigcuts

    def separate_points(self, strat, points, sel_size, boxes=None, max_parallel=None, pool_factor=4):
        """One separation round at EACH of several LP points of the bound instance in one device call (sdpcut_round_csr_points):
        the open nodes of a tree search, the children of a dive.  points [P, L + n]; strat 1, 2 or 4; sel_size as
        ``_sel_eigcut_by_ordering_on_measure`` takes it (a number of cuts).
        -> list of P tuples ``(csr, n_total, new_strat, counters)``: ``csr = (indptr, indices, values, rhs)`` is what
        :meth:`_gpu_add_csr` takes -- the caller adds each node's cuts to that node's LP -- and the rest is what the single-point
        selection reports (length of the ranking, the combined strategy's switch, its counters).  The arrays are views of the
        scorer's batch block, good until its next call; the scorer holds no current LP point afterwards.
        ``boxes`` [P, 2, n]: the variable bounds (lb, ub) of each point's node; entry p is then what ``set_box(*boxes[p])`` and
        the single-point round at ``points[p]`` give.  Still one device call (sdpcut_round_csr_points_boxed: every point's tables
        in its own box by one launch, one host wait for the batch -- DESIGN.md section 5 "Batched points"); the arrays are copies,
        and the solver's own node box (:meth:`set_node_box`), which the call cannot coexist with, is taken off the scorer before
        it and is in place again afterwards.
        ``max_parallel`` (None: the plain round above, unchanged): every point's round goes through the parallelism filter of
        :meth:`Scorer.round_csr_diverse` on a pool of ``min(pool_factor * sel_size, 16384)`` ranked candidates, still in one device
        call (sdpcut_round_csr_points_diverse); strat 1, 2, 4 or 6 (6 ranks by the efficacy score with the scorer's objective and
        weight).  Same hand-over form."""
        b = self._gpu_bind()
        b.drain()
        if max_parallel is not None:
            pool = int(min(max(int(pool_factor * int(sel_size)), int(sel_size)), _capi.DIVERSE_MAX_POOL))
            _capi.check_diverse_args(max_parallel, sel_size, pool, strat)

            def rounds_of(pts, copy, bx=None):
                return b.scorer.round_csr_points_diverse(pts, strat, sel_size, max_parallel, pool_size=pool, copy=copy, boxes=bx)
        else:
            def rounds_of(pts, copy, bx=None):
                return b.scorer.round_csr_points(pts, strat, sel_size, copy=copy, boxes=bx)
        if boxes is not None:
            pts = np.asarray(points, dtype=np.float64)
            bx = np.asarray(boxes, dtype=np.float64)
            if pts.ndim != 2 or bx.shape != (pts.shape[0], 2, self._nb_vars):
                raise ValueError("boxes must be [P, 2, n]: (lb, ub) per point")
            try:
                b.scorer.clear_box()
                rounds = rounds_of(pts, True, bx)
            finally:
                b.point_copy, b.scored, b.point_token = None, 0, None
                self._gpu_apply_box(b, self._gpu_node_box)
            return [((r["indptr"], r["indices"], r["values"], r["rhs"]), r["n_total"], r["new_strat"], r["counters"]) for r in rounds]
        rounds = rounds_of(points, False)
        b.point_copy, b.scored, b.point_token = None, 0, None      # (the next single-point selection uploads its point)
        return [((r["indptr"], r["indices"], r["values"], r["rhs"]), r["n_total"], r["new_strat"], r["counters"]) for r in rounds]

    def _gen_from_entries(self, entries, feas_sel, vars_values, pair):
        """Generic path for entries that do not carry a candidate index (random strategy, foreign
        lists): host gather of the tiny slices, GPU batched eigen-decomposition, row assembly."""
        L = self._nb_lifted
        vv = np.asarray(vars_values, dtype=np.float64)
        rows, rhs_out = [None] * len(entries), [None] * len(entries)
        by_k = {}
        for p, e in enumerate(entries):
            set_inds, Xarr_inds = (e[0], e[2]) if feas_sel else (e[0], e[1])
            by_k.setdefault(len(set_inds), []).append((p, set_inds, Xarr_inds))
        sc = self._gpu_any_scorer()
        for k, items in by_k.items():
            x = np.array([[vv[L + i] for i in it[1]] for it in items])
            X = np.array([[vv[i] for i in it[2]] for it in items])
            w, v = sc.eig_batch(k, x, X, want_vectors=True)
            for (p, set_inds, Xarr_inds), lam, vec in zip(items, w[:, 0], v[:, :, 0]):
                if lam < _THRES_NEG_EIGVAL:
                    ev = np.where(abs(vec) <= -_THRES_NEG_EIGVAL, 0, vec)
                    coef = [ev[a] * ev[c] * 2 if a != c else ev[a] * ev[c]
                            for a in range(k + 1) for c in range(max(a, 1), k + 1)]
                    rows[p] = pair(ind=[i + L for i in set_inds] + list(Xarr_inds), val=[float(t) for t in coef])
                    rhs_out[p] = float(-ev[0] * ev[0])
        rows_f = [r for r in rows if r is not None]
        rhs_f = [r for r in rhs_out if r is not None]
        self._my_prob.linear_constraints.add(lin_expr=rows_f, rhs=rhs_f, senses=["G"] * len(rows_f))
        return len(rows_f)

    def _gpu_any_scorer(self):
        for b in getattr(self, "_gpu_bindings", {}).values():
            return b.scorer
        if getattr(self, "_gpu_aux_scorer", None) is None:
            self._gpu_aux_scorer = _capi.Scorer(self._gpu_device)
        return self._gpu_aux_scorer

    # ------------------------------------------------------------------ triangle inequalities (8 f row 3)
    _THRES_TRI_VIOL = 10 ** (-7)
    _TRI_CUTS_PER_ROUND_MIN = 5000
    _TRI_CUTS_PER_ROUND_MAX = 10000

    def _gpu_dense_adj(self):
        """``self._Q_adj`` as a dense boolean array (the reference keeps a cvxopt spmatrix)."""
        adj = self._Q_adj
        if hasattr(adj, "I") and hasattr(adj, "J"):            # cvxopt.spmatrix
            out = np.zeros((self._nb_vars, self._nb_vars), dtype=bool)
            out[np.array(list(adj.I), dtype=int), np.array(list(adj.J), dtype=int)] = True
            return out
        if hasattr(adj, "a"):                                   # dense stand-in used by make_golden.py
            return np.asarray(adj.a) != 0
        return np.asarray(adj) != 0

    def _preprocess_triangle_ineq(self):
        """Triples to consider as triangle inequalities (cut_select_qp.py:799-822); the list
        lives on the device, the host keeps a copy for building the rows."""
        sc = _capi.Scorer(self._gpu_device)
        sc.set_instance(self._nb_vars, np.asarray(self._Q_arr, dtype=np.float64))
        self._gpu_tri = sc
        self._gpu_tri_triples, self._gpu_tri_density = sc.tri_preprocess(self._gpu_dense_adj())
        # the reference's bookkeeping lists, for code that only looks at their length
        self._idx_list_tri = self._gpu_tri_triples
        self._gpu_tri_triples64 = None
        self._rank_list_tri = None

    def _separate_and_add_triangle(self, sel_size, vars_values):
        """Separate the violated triangle inequalities at the current point, rank them by
        (density, violation) and append the selected ones (cut_select_qp.py:824-863)."""
        sc, tri, L, n = self._gpu_tri, self._gpu_tri_triples, self._nb_lifted, self._nb_vars
        sc.set_point(_lp_point(vars_values))
        ent, vio, nb_viol = sc.tri_separate(self._TRI_CUTS_PER_ROUND_MAX)
        nb_tri_cuts = max(min(self._TRI_CUTS_PER_ROUND_MIN, int(np.floor(sel_size * nb_viol))),
                          min(self._TRI_CUTS_PER_ROUND_MAX, nb_viol))                       # :844-845
        if nb_tri_cuts <= 0:
            return self._gpu_add_csr(None)
        # the rows as ONE CSR block built with array operations (the per-row Python loop of :847-861 cost ~3 us per cut, 30 ms for
        # the 10 000 cuts of a round -- two orders of magnitude more than the device took to find them): inequality c of triple
        # (a, b, d) has columns X_ab, X_ad, X_bd and x_(a|b|d)[c]  (c < 3: 4 non-zeros, rhs 0) or x_a, x_b, x_d (c = 3: 6, rhs -1)
        e = np.asarray(ent[:nb_tri_cuts], dtype=np.int64)
        c = (e & 3).astype(np.int64)
        tri64 = getattr(self, "_gpu_tri_triples64", None)
        if tri64 is None or tri64.shape[0] != len(tri):
            tri64 = self._gpu_tri_triples64 = np.asarray(tri, dtype=np.int64)      # (converted once: 80 us per round otherwise)
        abd = tri64[e >> 2]
        a3, b3, d3 = abd[:, 0], abd[:, 1], abd[:, 2]
        ra, rb = n * a3 - a3 * (a3 + 1) // 2, n * b3 - b3 * (b3 + 1) // 2
        four = c < 3
        indptr = np.zeros(e.shape[0] + 1, dtype=np.int64)
        np.cumsum(np.where(four, 4, 6), out=indptr[1:])
        pos = indptr[:-1]
        ind = np.empty(int(indptr[-1]), dtype=np.int64)
        val = np.empty(int(indptr[-1]), dtype=np.float64)
        ind[pos], ind[pos + 1], ind[pos + 2] = ra + b3, ra + d3, rb + d3            # Xarr_inds[1], [2], [4]
        p4, p6 = pos[four], pos[~four]
        ind[p4 + 3] = abd[four, c[four]] + L
        ind[p6 + 3], ind[p6 + 4], ind[p6 + 5] = a3[~four] + L, b3[~four] + L, d3[~four] + L
        v4 = np.array([[-1.0, -1.0, 1.0, 1.0], [-1.0, 1.0, -1.0, 1.0], [1.0, -1.0, -1.0, 1.0]])[c[four]]
        for j in range(4):
            val[p4 + j] = v4[:, j]
        for j, v in enumerate((1.0, 1.0, 1.0, -1.0, -1.0, -1.0)):
            val[p6 + j] = v
        # (built here: no second copy; the reference hands integer coefficients and right-hand sides, :833-836)
        return self._gpu_add_csr((indptr, ind, val, np.where(four, 0.0, -1.0)), copy=False, integral=True)

    def _separate_and_add_triangle_node(self, sel_size, vars_values):
        """The triangle step of a run at a node (``cut_select_algo(box=..., triangle_on=True, triangle_box=True)``): the
        inequalities of the NODE'S box -- the facets in ``x' = (x - l) / d``, ``X'``, mapped back to rows in the original
        variables (:mod:`triangles`) -- separated, ranked and assembled on the device (``Scorer.tri_round_csr`` on the triangle
        handle, which holds the run's box).  The number of cuts follows the reference's rule (:844-845) on the node's count."""
        r = self._gpu_tri.tri_round_csr(self._TRI_CUTS_PER_ROUND_MAX, point=_lp_point(vars_values))
        nb_viol = r["n_violated"]
        nb_tri_cuts = min(max(min(self._TRI_CUTS_PER_ROUND_MIN, int(np.floor(sel_size * nb_viol))),
                              min(self._TRI_CUTS_PER_ROUND_MAX, nb_viol)), r["n_rows"])
        if nb_tri_cuts <= 0:
            return self._gpu_add_csr(None)
        indptr = r["indptr"][:nb_tri_cuts + 1]
        nnz = int(indptr[-1])
        return self._gpu_add_csr((indptr, r["indices"][:nnz], r["values"][:nnz], r["rhs"][:nb_tri_cuts]), copy=True)

    def separate_triangles_points(self, points, max_cuts, boxes=None):
        """The triangle inequalities at P LP points in one device call with one host wait (``Scorer.tri_round_csr_points``): the
        open nodes of a tree search.  points [P, n(n+1)/2 + n]; boxes [P, 2, n] = (lb, ub) of every point's node, or None (the
        root's inequalities everywhere).  -> list of P ``(csr, n_violated)``: csr = (indptr, indices, values, rhs) of the first
        ``max_cuts`` violated inequalities of point p in rank order, sense >=, as :meth:`_gpu_add_csr` takes them (copies: they
        outlive the next call); n_violated the length of the full list.  The call keeps a handle of its own with the triples
        of the bound instance's pattern (``self._Q_adj``): the triangle handle of a running loop, which may hold the run's box,
        is not touched."""
        adj = np.ascontiguousarray(self._gpu_dense_adj(), dtype=np.uint8)
        key = (self._nb_vars, adj.tobytes())
        if getattr(self, "_gpu_tri_points_key", None) != key:
            if getattr(self, "_gpu_tri_points", None) is not None:      # another pattern: the old handle goes first
                self._gpu_tri_points.close()
                self._gpu_tri_points = self._gpu_tri_points_key = None
            sc = _capi.Scorer(self._gpu_device)
            sc.set_instance(self._nb_vars, np.asarray(self._Q_arr, dtype=np.float64))
            sc.tri_preprocess(adj)
            self._gpu_tri_points, self._gpu_tri_points_key = sc, key
        res = self._gpu_tri_points.tri_round_csr_points(points, int(max_cuts), boxes=boxes, copy=True)
        return [((r["indptr"], r["indices"], r["values"], r["rhs"]), r["n_violated"]) for r in res]

    def separate_pool_points(self, points, max_cuts, viol_tol=1e-6, pool=None):
        """A cut pool separated at P LP points in one device call with one host wait, read-only
        (``Scorer.pool_separate_points`` with ``states="all"``): the open nodes of a tree search ask a GLOBAL pool first, before
        their own separators run.  points [P, n(n+1)/2 + n]; ``pool``: a ``Scorer`` with a pool or a :class:`cutpool.CutPoolTwin`,
        by default ``self.pool_loop.pool`` -- the pool a ``cut_select_algo(pool_max_age=...)`` run leaves behind, with the
        eigen-cuts of that run.  -> list of P ``(csr, sense, serials, n_violated)``: csr = (indptr, indices, values, rhs) of the
        first ``max_cuts`` rows point p violates by more than ``viol_tol * ||row||``, most violated first, as
        :meth:`_gpu_add_csr` takes them; sense +1 (>=) / -1 (<=) per row (``_gpu_add_csr`` adds >= rows: a <= row is negated by
        the caller); the rows' serials (what ``pool_drop`` takes); n_violated the length of the full list.  The arrays are copies.
        The pool, its states and ages, and the scorer's LP point are left as they were.

        Only GLOBALLY valid rows belong in a pool that is asked at other nodes: eigen-cuts and the root's triangle inequalities
        are; rows valid only inside a node's box -- the rows of ``triangle_box=True`` -- must not be pooled globally.  Nothing
        checks that."""
        if pool is None:
            loop = getattr(self, "pool_loop", None)
            if loop is None:
                raise ValueError("no pool: pass pool= or run cut_select_algo(pool_max_age=...) first")
            pool = loop.pool
        res = pool.pool_separate_points(points, int(max_cuts), viol_tol=viol_tol, states="all", copy=True)
        return [((r["indptr"], r["indices"], r["values"], r["rhs"]), r["sense"], r["serial"], r["n_violated"]) for r in res]

    def evaluate_points(self, points, boxes=None, obj=None, **kw):
        """Node evaluation at P LP points of the bound instance in one device call with one host wait, read-only
        (``Scorer.node_eval_points``, :mod:`nodeeval`): per point an incumbent by coordinate descent from the projected LP point,
        the true objective there and a branching variable with its value.  points [P, n(n+1)/2 + n]; boxes [P, 2, n] = (lb, ub)
        of every point's node or None; ``kw``: max_sweeps, branch_rule, rho.  The objective is the bound LP's own vector
        ``self._my_prob.obj`` = [Q_arr | c] -- handed to the handle the way strategy 6 hands it over, once per vector -- or ``obj``.
        -> the dict of arrays ``Scorer.node_eval_points`` returns (copies).  The scorer's point, scores and box stay as they were."""
        b = self._gpu_bind()
        if obj is None:
            lp = getattr(self, "_my_prob", None)
            if lp is None or getattr(lp, "obj", None) is None:
                raise ValueError("evaluate_points: no LP is bound (self._my_prob) and no obj= is given")
            obj = lp.obj
        obj = np.ascontiguousarray(obj, dtype=np.float64)
        if b.scorer.objective_key != obj.tobytes():      # (the Scorer knows what it holds, whoever set or cleared it)
            b.drain()
            b.scorer.set_objective(obj)
            b.scored &= ~_capi.EFF      # (the library drops the efficacy scores of the old vector)
        return b.scorer.node_eval_points(points, boxes=boxes, copy=True, **kw)

    # the reference reaches these two through name-mangled private names inside class CutSolver
    _CutSolver__preprocess_triangle_ineq = _preprocess_triangle_ineq
    _CutSolver__separate_and_add_triangle = _separate_and_add_triangle

    # ------------------------------------------------------------------ a6 eigen helper
    def _get_eigendecomp(self, dim_subpr, curr_pt, X_slice, ev_yes):
        """Eigen-decomposition of [[1, x^T],[x, X]] (cut_select_qp.py:788-797): ascending
        eigenvalues, and eigenvectors as columns when ``ev_yes`` (numpy's eigh layout)."""
        sc = self._gpu_any_scorer()
        x = np.asarray(curr_pt, dtype=np.float64)[None, :]
        X = np.asarray(X_slice, dtype=np.float64)[None, :]
        if ev_yes:
            w, v = sc.eig_batch(dim_subpr, x, X, want_vectors=True)
            return w[0], v[0]
        return sc.eig_batch(dim_subpr, x, X)[0]


class CutSolver(GpuCutSelectionMixin):
    """Stand-alone twin of the reference's ``CutSolver`` state (cut_select_qp.py:43-71) for use
    without the reference installed: holds the instance tables and the candidate list, and
    exposes the four GPU-backed hot-path methods.  The constants keep the reference's names."""
    _THRES_MIN_OPT = 0
    _THRES_NEG_EIGVAL = _THRES_NEG_EIGVAL
    _BIG_M = _BIG_M
    _SDP_CUTS_PER_ROUND_MAX = 5000
    _THRES_MAX_SUBS = 4 * (10 ** 6)

    def __init__(self, device=0, exact_heads=False, exact_sdp=False):
        self._gpu_device = device
        self._gpu_exact_heads = bool(exact_heads)
        self._gpu_exact_sdp = bool(exact_sdp)
        self._dim = 0
        self._nb_vars = 0
        self._nb_lifted = 0
        self._Q_arr = []
        self._my_prob = None
        self._agg_list = []
        self._nns = None

    def set_instance(self, nb_vars, Q_arr, agg_list, dim, my_prob=None):
        """Bind an instance: packed objective, candidate records (reference layout, only
        ``[0]`` = set_inds and ``[1]`` = Xarr_inds of each record are read) and the LP object."""
        assert dim <= 5, "Keep SDP vertex cover low-dimensional (<=5)!"      # cut_select_qp.py:93
        self._nb_vars, self._nb_lifted = nb_vars, nb_vars * (nb_vars + 1) // 2
        self._Q_arr, self._agg_list, self._dim = Q_arr, agg_list, dim
        self._my_prob = my_prob
        self._load_neural_nets()

    @staticmethod
    def selection_size(sel_size, nb_subprobs, minimum=0):
        """sel_size rule of cut_select_qp.py:123-125 (QCQP adds `minimum=1`, cut_select_qcqp.py:57-58)."""
        assert 0 < sel_size, "The selection size must be a % or number (of cuts) >0!"
        s = min(int(np.floor(sel_size * nb_subprobs)) if sel_size < 1 else min(sel_size, nb_subprobs),
                CutSolver._SDP_CUTS_PER_ROUND_MAX)
        return max(s, minimum)

    # ------------------------------------------------------------------ rounds without CPLEX (SURVEY 8 f row 2)
    _CONVERGENCE_TOL = 10 ** (-3)         # cut_select_qp.py:29

    # the separation step between two LP solves of cut_select_algo, one function per kind of round; they read the run's
    # settings from self._run and return the round's counts
    def _round_counts(self, sdp, point):
        """the counts of a round that added ``sdp`` eigen-cuts: the triangle inequalities are separated behind them"""
        run = self._run
        if not run.triangle_on:
            return {"sdp": sdp, "tri": 0}
        tri_step = self._separate_and_add_triangle_node if getattr(run, "triangle_box", False) else self._separate_and_add_triangle
        return {"sdp": sdp, "tri": tri_step(run.sel_size, point)}

    def _round_plain(self, round_no, point):
        """selection, then generation, as the reference's loop calls them (cut_select_qp.py:165-182)"""
        run = self._run
        cur = run.strat
        if cur == 0:
            return self._round_counts(self._gen_dense_eigcuts(vars_values=point), point)
        picked = self._sel_eigcut_by_ordering_on_measure(cur, point, round_no, **({"sel_size": run.quota} if cur in (4, -1) else {}))
        if cur == 4 and isinstance(picked, tuple):
            run.strat, picked = picked            # the switch takes effect next round (:181 vs :188)
        if cur == -1:                             # :173-179
            picked, round_stats, round_std_dev, round_all_cuts = picked
            run.figure8[0].append(round_stats)
            run.figure8[1].append(round_std_dev)
            run.figure8[2].extend(round_all_cuts)
        sdp = self._gen_eigcuts_selected(cur, run.quota, picked, strong_only=run.strong_only, vars_values=point)
        return self._round_counts(sdp, point)

    def _round_one_call(self, round_no, point):
        """a round whose ranking and assembled cuts come from ONE library call: through the parallelism filter (``max_parallel``),
        or with all violated eigen-cuts of the selected sets (``cuts_per_set`` > 1)"""
        run = self._run
        cur = run.strat
        if cur == 5 or run.quota < 1:
            return self._round_plain(round_no, point)     # (strategy 5: _gen_eigcuts_selected sees self.cuts_per_set)
        multi = run.m_cuts > 1
        b = self._gpu_bind()
        b.drain()
        vv = _lp_point(point)
        if multi:
            r = b.scorer.round_csr_multi(b.point_arg(vv), cur, run.quota, run.m_cuts, row_quota=run.row_quota)
        else:
            pool = int(min(max(int(run.pool_factor * run.quota), run.quota), _capi.DIVERSE_MAX_POOL))
            r = b.scorer.round_csr_diverse(b.point_arg(vv), cur, run.quota, run.max_parallel, pool_size=pool)
        b.note_point(vv, _MEASURES[cur])
        b.rank_serial += 1
        self._gpu_last = None
        if cur == 4:
            run.strat = r["new_strat"]            # the switch takes effect next round (:181 vs :188)
        entries = int(r["idx"].shape[0])
        csr = csr_prefix(r, strong_prefix(r["score"], entries) if run.strong_only and cur in _STRONG_STRATS else entries)      # :725-726
        if multi:
            rows = csr[3].shape[0]
            used = r["row_entry"][:rows]
            self._multi_log_add(round=round_no, strat=cur, entries=entries, entries_used=int(np.unique(used).shape[0]),
                                last_entry=int(used[-1]) + 1 if rows else 0, rows=rows, n_neg_hist=np.bincount(r["n_neg"], minlength=6).tolist(),
                                quota=int(r["row_cap"]), quota_hit=bool(r["quota_hit"]))
        else:
            self.diverse_log.append(dict(r["info"], round=round_no, strat=cur, accepted=entries))
        return self._round_counts(self._gpu_add_csr(csr), point)

    def _round_pooled(self, round_no, point):
        """the pool's step first (its upload of the point serves the round), then the round; its rows join the pool"""
        run = self._run
        ploop = run.pool
        vv = _lp_point(point)
        b = self._gpu_bind() if run.strat != 5 else None
        if b is not None:
            b.drain()
        ploop.step(vv, run.pool_return)
        if b is not None and b.scorer is ploop.pool:
            b.note_point(vv, 0)
            b.point_fresh = True
        counts = run.unpooled(round_no, point)
        ploop.adopt()
        return dict(counts, pool_enter=ploop.log[-1]["enter"], pool_leave=ploop.log[-1]["leave"])

    def cut_select_algo(self, filename, dim, sel_size, strat=2, nb_rounds_cuts=20, term_on=False,
                        triangle_on=False, strong_only=False, max_subs=_THRES_MAX_SUBS, on_round=None, plots=False, sol=0,
                        ch_ext=0, max_parallel=None, pool_factor=4, cuts_per_set=1, row_quota=None,
                        pool_max_age=None, pool_drop_age=10, pool_return=None, pool_tight_tol=1e-9, pool_viol_tol=1e-6, box=None,
                        objpar_weight=0.0, triangle_box=False):
        """Cutting-plane rounds on a BoxQP ``.in`` file, same arguments and default return tuple as
        the reference's entry point (cut_select_qp.py:73-221), with HiGHS as LP solver, the native
        cover enumeration and the GPU selection / generation / triangle separation in between.
        ``max_subs=None`` lifts the reference's 4e6 candidate guard (:117-120); ``on_round(r, log)`` is
        called after every LP solve (progress of long runs).  Strategy 0 adds
        the fully dense eigen-cuts of :meth:`_gen_dense_eigcuts` instead of a selection (the cover is still enumerated: the tuple
        reports its size).  ``ch_ext`` (:84): 0 = P^E_dim, 1 = P^bar(E)_dim, 2 = bar(P*_3), the covers on a chordal extension of
        the sparsity pattern -- the elimination game under greedy minimum degree (``_capi.chordal_extension``), not cvxopt's AMD,
        so the number of candidates can differ from the published one.  As in the reference once ``self._Q_adj`` is replaced
        (:396), the McCormick rows and the triangle inequalities then use the EXTENDED pattern, which ``self._Q_adj`` holds
        afterwards.  ``ch_ext=2`` needs ``dim=3`` (the reference silently degrades it to ``ch_ext=1`` at dim 4 and 5; here it is
        refused).  ``CutSolver(exact_sdp=True)`` also takes strategy 3
        (optimality via the exact SDP solution) and -1 (figure 8); with ``strat=-1, plots=True`` the return is the reference's
        ``(gap_closed_percent, rounds_stats, round_std_devs, rounds_all_cuts)`` with the gap closed measured against ``sol``
        (:209-215).  ``plots`` with another strategy is out of scope.
        Strategy 6 (not the reference's) ranks all candidates by the EFFICACY of the eigen-cut they would emit -- the distance by
        which the row cuts off the LP point, the first criterion of a MIP solver's cut selector -- plus ``objpar_weight`` (>= 0,
        default 0; SCIP's default weights correspond to 0.1) times the row's parallelism to the LP objective (``Scorer.score(EFF)``,
        DESIGN.md section 5 "Efficacy ranking"); with a positive weight the run hands its LP's objective vector to the handle.  No
        networks are loaded; ``strong_only`` has no meaning there and is ignored; ``max_parallel`` and ``cuts_per_set`` work with it.
        ``CutSolver(exact_sdp=True)`` refuses it as before: that opt-in's strategy set is unchanged.
        ``max_parallel`` (off by default; strategies 1, 2, 4 and 6 only): a parallelism filter on the ranked head
        (``Scorer.round_csr_diverse``, DESIGN.md section 5 "Diverse selection").  Each round walks the first
        ``min(pool_factor * quota, 16384)`` ranked candidates and adds a cut only while fewer than the quota are added and its
        ``|cos|`` with every cut added before it in the round is at most ``max_parallel``; the walk's counts of every round are
        kept in ``self.diverse_log``.  The combined strategy's switch and ``strong_only`` work as without the filter.
        ``cuts_per_set`` (1 = today's round, untouched; up to 5; not with strategy 0 or -1, not with ``max_parallel``): every
        selected set offers all its violated eigen-cuts, at most that many (``Scorer.round_csr_multi``, DESIGN.md section 5 "All
        violated eigen-cuts"; strategy 5 through ``Scorer.cut_rows_all``).  ``row_quota=None`` keeps the LP budget of a plain round
        -- at most ``quota`` rows, so fewer sets are used -- and ``row_quota="sets"`` lets every one of the ``quota`` sets keep all
        it offers (up to ``cuts_per_set * quota`` rows).  ``self.multi_log`` records every round: entries used, rows, the
        histogram of violated eigenvalues per entry, whether the quota dropped a row.
        ``pool_max_age`` (None = no pool, today's loop untouched; not with strategy 0): a cut pool on the device
        (``Scorer.pool_*``, DESIGN.md section 5 "Cut pool").  Every round begins with one pool step at the LP point: a cut that
        has been slack by more than ``pool_tight_tol * ||row||`` at ``pool_max_age`` consecutive LP optima leaves the LP and is
        parked; parked cuts violated by more than ``pool_viol_tol * ||row||`` return, most violated first, at most
        ``pool_return`` of them (None = the round's quota; they do not count against it); a cut parked for ``pool_drop_age``
        rounds is dropped.  Then the usual separation runs and its rows -- eigen-cuts and triangle rows, never the McCormick
        rows -- go into both the LP and the pool.  ``self.pool_log`` has one record per round: leave, enter, dropped, in_lp, parked
        (after the step), violated, lp_rows (rows of the LP that was just solved), added (rows the separation added).
        ``box=(lb, ub)`` (scalars or [n] arrays; None = the root): the same loop at a branch-and-bound node with the variable bounds
        ``lb <= x <= ub`` -- the LP is the node's relaxation (``harness.boxqp_relaxation(inst, lb, ub)``) and the optimality
        measures are the node's (``Scorer.set_box`` on the run's own handle, DESIGN.md section 5 "Node boxes").  The run's box is
        this argument alone: a box set with :meth:`set_node_box` is neither used nor changed.
        ``triangle_box`` (False = today's triangle step, untouched; needs ``box`` and ``triangle_on``, ValueError otherwise): the
        triangle step separates the inequalities of the NODE'S box instead of the unit box's -- the same facets in the box's own
        variables, which are valid at the node and tighter, as rows in the original variables assembled on the device
        (``Scorer.tri_round_csr``, DESIGN.md section 5 "Triangle inequalities at nodes").
        -> (bound per solve, total s, round s, separation s, PSD cuts per round, triangle cuts per
        round, number of candidates)."""
        from timeit import default_timer as clock
        from . import harness
        if strat == 6 and self._gpu_exact_sdp:      # the opt-in's strategy set stays what it was: 6 was refused there and still is
            raise AssertionError("strategy 6 (efficacy) is offered by the default solver only: CutSolver(exact_sdp=True) keeps its strategies "
                                 "0, 1, 2, 3, 4, 5 and -1")
        if strat not in (0, 1, 2, 4, 5, 6) and not (self._gpu_exact_sdp and strat in (3, -1)):
            raise AssertionError("strategies on the GPU path: 0 dense, 1 feasibility, 2 optimality, 4 combined, 5 random, 6 efficacy "
                                 "(3 exact optimality and -1 figure 8 with exact_sdp=True)")
        objpar_weight = float(objpar_weight)
        assert 0.0 <= objpar_weight < float("inf"), "objpar_weight is the weight of the objective parallelism in strategy 6's score: finite, >= 0"
        assert objpar_weight == 0.0 or strat == 6, "objpar_weight belongs to strategy 6 (efficacy)"
        assert not plots or strat == -1, "plots=True returns the figure-8 tuple: strat=-1 only"
        assert 0 < sel_size, "The selection size must be a % or number (of cuts) >0!"
        assert dim <= 5, "Keep SDP vertex cover low-dimensional (<=5)!"
        assert (ch_ext in [0, 1, 2]), "Chordal extension flags: 0-P^E_3, 1-P^bar(E)_3, 2-bar(P*_3)!"      # :94
        if ch_ext == 2 and dim != 3:      # (with the other argument checks: before the file is read and a handle is made)
            raise ValueError("ch_ext = 2 is a cover of dimension 3 only")
        if triangle_box and (box is None or not triangle_on):
            raise ValueError("triangle_box switches the triangle step of a node's run to the node's inequalities: it needs box= and triangle_on=True")
        if max_parallel is not None:
            if strat not in (1, 2, 4, 6):
                raise AssertionError("max_parallel filters the ranked head of strategies 1 (feasibility), 2 (optimality), 4 (combined) and 6 (efficacy) only")
            assert 0.0 <= max_parallel <= 1.0, "max_parallel is a bound on |cos| between two cuts: 0 .. 1"
            assert pool_factor >= 1, "the pool is pool_factor times the quota: pool_factor >= 1"
            self.diverse_log = []
        m_cuts, _ = _capi.check_multi_args(cuts_per_set, 1)
        if m_cuts > 1:
            if max_parallel is not None:
                raise AssertionError("cuts_per_set > 1 together with max_parallel is not offered")
            if strat in (0, -1):
                raise AssertionError("cuts_per_set > 1 serves the selecting strategies 1, 2, 3, 4 and 5 (strategy 0 emits every dense cut already)")
            assert row_quota in (None, "sets"), 'row_quota is None (the round\'s quota in rows) or "sets" (cuts_per_set times the quota)'
            self.multi_log = []
        pooled = pool_max_age is not None
        if pooled:
            if strat == 0:
                raise AssertionError("the cut pool holds sparse rows of at most 20 entries: strategy 0 (dense cuts) is not pooled")
            pool_par = _capi.check_pool_params(pool_tight_tol, pool_viol_tol, pool_max_age, pool_drop_age,
                                               0 if pool_return is None else pool_return)
            assert nb_rounds_cuts >= 0
        t_start = clock()
        inst = harness.parse_boxqp(filename)
        self._dim = dim
        self._nb_vars, self._nb_lifted, self._Q_arr, self._Q_adj = (inst[k] for k in ("nb_vars", "nb_lifted", "Q_arr", "adj"))
        self._gpu_nets = {}
        if strat in (2, 4, -1):      # :103
            self._load_neural_nets()
        # the cover is enumerated on the device, straight into the scorer's candidate list
        sc = self._gpu_new_scorer()
        sc.set_instance(self._nb_vars, np.asarray(self._Q_arr, dtype=np.float64))
        node_box = None if box is None else self._gpu_check_box(*box)      # (the run's own: set_node_box's is left alone)
        if node_box is not None:
            sc.set_box(*node_box)
        n_cand = sc.set_candidates_cover(inst["adj"], dim, max_subs=max_subs or 0, ch_ext=ch_ext)
        if ch_ext:      # :396 -- everything after the cover sees the extended pattern
            inst = dict(inst, adj=_capi.chordal_extension(inst["adj"])[0])
            self._Q_adj = inst["adj"]
        if (max_subs and n_cand >= max_subs) or nb_rounds_cuts == 0:
            sc.close()
            return [0, 0], clock() - t_start, 0, 0, [0], 0, n_cand                      # the reference's guard tuple
        self._agg_list = DeviceAgg(sc, n_cand, self._nb_vars, self._Q_arr)
        quota = self.selection_size(sel_size, n_cand)
        t_model = clock()
        self._my_prob = lp = harness.boxqp_relaxation(inst, *(node_box or ()))
        t_model = clock() - t_model
        if strat == 6:
            sc.set_efficacy_weight(objpar_weight)
            if objpar_weight > 0.0:
                sc.set_objective(lp.obj)      # [Q_arr | c]: the LP's columns are the LP point's
        if triangle_on:
            self._preprocess_triangle_ineq()
            if triangle_box:
                self._gpu_tri.set_box(*node_box)
        rounds_stats, round_std_devs, rounds_all_cuts = [], [], []      # figure 8 (:144)
        if strat == 0:      # the cover's scorer already holds the instance
            self._gpu_dense_sc, self._gpu_dense_key = sc, (self._nb_vars, id(self._Q_arr))
        # what the round functions read, and the strategy they update (the combined strategy's switch)
        self._run = run = SimpleNamespace(strat=strat, quota=quota, sel_size=sel_size, triangle_on=triangle_on, strong_only=strong_only,
                                          max_parallel=max_parallel, pool_factor=pool_factor, m_cuts=m_cuts, row_quota=row_quota,
                                          triangle_box=bool(triangle_box), figure8=(rounds_stats, round_std_devs, rounds_all_cuts))
        sep_fn = self._round_plain if m_cuts == 1 and max_parallel is None else self._round_one_call
        if pooled:
            from . import cutpool
            # capacity = the most rows the run can add: there is no eviction under pressure
            per_round = quota * (m_cuts if row_quota == "sets" else 1) + (self._TRI_CUTS_PER_ROUND_MAX if triangle_on else 0)
            capacity = max(1, nb_rounds_cuts * per_round)
            if capacity > _capi.POOL_MAX_ROWS:
                raise ValueError("the run can add %d rows, a cut pool holds at most %d" % (capacity, _capi.POOL_MAX_ROWS))
            sc.pool_create(capacity)
            ploop = cutpool.PoolLoop(lp, sc, pool_par[2], pool_par[3], pool_par[0], pool_par[1])
            self.pool_log, self.pool_loop = ploop.log, ploop
            run.pool, run.pool_return, run.unpooled = ploop, quota if pool_return is None else pool_par[4], sep_fn
            sep_fn = self._round_pooled
        keep_attr = (self.cuts_per_set, self.cuts_row_quota)
        if m_cuts > 1:
            self.cuts_per_set, self.cuts_row_quota = m_cuts, row_quota
        try:
            log = harness.run_cut_rounds(lp, sep_fn, nb_rounds_cuts, setup_s=t_model,
                                         stop_tol=self._CONVERGENCE_TOL if term_on else None, on_round=on_round,
                                         after_solve=self._gpu_wake,
                                         # dense cuts: past the 4th round, stop once the rounds have taken 1000 s (:157)
                                         stop=(lambda r, lg: r > 4 and sum(lg.solve_s) + sum(lg.separation_s) > 1000) if strat == 0 and term_on else None)
        finally:
            self.cuts_per_set, self.cuts_row_quota = keep_attr
        sep = [t_model] + log.separation_s
        if plots:       # :209-215 (curr_obj_vals of the reference = log.bounds)
            gap_closed_percent = [0] + [(-v + log.bounds[0]) / (sol + log.bounds[0]) for v in log.bounds[1:]]
            return gap_closed_percent, rounds_stats, round_std_devs, rounds_all_cuts
        return ([-v for v in log.bounds], clock() - t_start, [a + b for a, b in zip(log.solve_s, [0.0] + log.separation_s)],
                sep, [0] + log.column("sdp"), log.column("tri"), n_cand)

    def branch_and_cut(self, filename, dim, sel_size, strat=2, triangles=True, triangle_box=True, boxes=True, max_subs=_THRES_MAX_SUBS,
                       tri_cuts=1000, wrap=None, **kw):
        """Best-first branch and cut on a BoxQP ``.in`` file with the device's batched node calls (:func:`tree.branch_and_cut` with
        :func:`tree.gpu_backends`): per iteration one ``separate_points`` round of strategy ``strat`` (1, 2, 4; ``sel_size`` as
        ``cut_select_algo`` takes it) and, with ``triangles``, one ``separate_triangles_points`` call per separation round, and one
        ``evaluate_points`` call, for all nodes of the batch.  ``boxes``: the optimality measure of every node in its own box;
        ``triangle_box``: the triangle inequalities of every node's box; at most ``tri_cuts`` triangle rows per node and round.
        ``kw``: batch, rounds, gap_tol, max_nodes, time_limit, branch_rule, rho, max_sweeps.  ``wrap(separate, evaluate)`` may
        return the pair the driver is to call instead (tools and tests that record what passes through).
        -> ``tree.TreeResult`` (values in the LP's minimising form, ``sign = -1``: the file maximises) with ``n_candidates``."""
        from . import harness, tree
        if strat not in (1, 2, 4):
            raise AssertionError("branch_and_cut separates with strategies 1 (feasibility), 2 (optimality) and 4 (combined)")
        inst = harness.parse_boxqp(filename)
        self._dim = dim
        self._nb_vars, self._nb_lifted, self._Q_arr, self._Q_adj = (inst[k] for k in ("nb_vars", "nb_lifted", "Q_arr", "adj"))
        self._gpu_nets = {}
        if strat in (2, 4):
            self._load_neural_nets()
        sc = self._gpu_new_scorer()
        sc.set_instance(self._nb_vars, np.asarray(self._Q_arr, dtype=np.float64))
        n_cand = sc.set_candidates_cover(inst["adj"], dim, max_subs=max_subs or 0)
        self._agg_list = DeviceAgg(sc, n_cand, self._nb_vars, self._Q_arr)
        self._my_prob = harness.boxqp_relaxation(inst)      # (its objective vector is what evaluate_points hands to the handle)
        quota = self.selection_size(sel_size, n_cand, minimum=1)
        ev = {k: kw[k] for k in ("branch_rule", "rho", "max_sweeps") if k in kw}
        separate, evaluate = tree.gpu_backends(self, strat=strat, sel_size=quota, triangles=triangles, triangle_box=triangle_box,
                                               boxes=boxes, tri_cuts=tri_cuts, **ev)
        if wrap is not None:
            separate, evaluate = wrap(separate, evaluate)
        res = tree.branch_and_cut(inst, separate, evaluate, sign=-1.0, **kw)
        res.n_candidates = n_cand
        return res


class CutSolverQCQP(CutSolver):
    """QCQP composition of the path (cut_select_qcqp.py:63-103): the objective cover is ranked
    with ``strat``, the constraint-only cover with feasibility, the lists are concatenated."""

    def select_and_generate_round(self, strat, vars_values, cut_round, sel_size, agg_list, agg_list_cons):
        """One round of cut_select_qcqp.py:64-98.  Returns
        (new_strat, rank_list, nb_sdp_cuts, nb_opt_cuts)."""
        strat_old = strat
        self._agg_list = agg_list
        if strat == 5:
            rank_list = self._sel_eigcut_by_ordering_on_measure(strat, vars_values, cut_round)
            return strat, rank_list, self._gen_eigcuts_selected(strat, sel_size, rank_list,
                                                                vars_values=vars_values), 0
        if strat == 4:
            strat, comb_obj = self._sel_eigcut_by_ordering_on_measure(strat, vars_values, cut_round,
                                                                      sel_size=sel_size)
        else:
            comb_obj = self._sel_eigcut_by_ordering_on_measure(strat, vars_values, cut_round)
        self._agg_list = agg_list_cons                       # :75
        feas_cons = self._sel_eigcut_by_ordering_on_measure(1, vars_values, cut_round)
        self._agg_list = agg_list                            # :78
        n_obj = min(len(comb_obj), sel_size)
        rank_list = comb_obj[0:n_obj] + feas_cons[0:sel_size - n_obj]      # == (A + B)[0:sel_size], :79
        if strat_old == 1:
            nb = self._gen_eigcuts_selected(strat_old, sel_size, rank_list, vars_values=vars_values)
            return strat, rank_list, nb, 0
        # :85-92 counters, from the device arrays instead of a Python loop over N tuples
        nb_opt_cuts = (comb_obj.count_above(_BIG_M) if isinstance(comb_obj, RankList) else
                       int(np.count_nonzero(np.array([e[1] for e in comb_obj]) > _BIG_M))) if len(comb_obj) else 0
        if int(self.cuts_per_set) > 1:
            # all violated eigen-cuts: ONE walk over the concatenated head, so that the row quota is applied in list order
            return strat, rank_list, self._gen_eigcuts_selected(strat_old, sel_size, rank_list, vars_values=vars_values), nb_opt_cuts
        nb_cuts_combined = n_obj      # :90-92 counts the entries whose first field is an int: the objective cover's (optimality / combined entries)
        rest = sel_size - nb_cuts_combined
        nb_a = self._gen_eigcuts_selected(1, rest, feas_cons[0:rest], vars_values=vars_values)
        nb_b = self._gen_eigcuts_selected(strat_old, nb_cuts_combined, comb_obj[0:nb_cuts_combined],
                                          vars_values=vars_values)
        return strat, rank_list, nb_a + nb_b, nb_opt_cuts

    def _round_qcqp(self, round_no, point):
        """the separation step between two LP solves of the QCQP loop"""
        run = self._run
        run.strat, _, sdp, opt = self.select_and_generate_round(run.strat, point, round_no, run.quota, *run.covers)
        return {"sdp": sdp, "opt": opt}

    def cut_select_algo(self, filename, dim, sel_size=0.1, strat=2, nb_rounds_cuts=20, cuts_per_set=1):
        """Cutting-plane rounds on a QCQP in OSiL format, same arguments and return tuple as the
        reference's QCQP entry point (cut_select_qcqp.py:16-113), with HiGHS, the native enumeration
        of both covers and :meth:`select_and_generate_round` between two solves.
        ``cuts_per_set`` > 1: the two-handle selection runs as before, then each handle emits up to that many eigen-cuts for its
        part of the concatenated head (``Scorer.cut_rows_all``) and the first ``sel_size`` rows in list order are kept
        (``self.multi_log`` has one record per round).
        -> (objective value per solve, sel_size, PSD cuts per round, optimality cuts per round)."""
        from . import harness
        if strat == 6:
            raise AssertionError("strategy 6 (efficacy) is not offered for QCQP: ranking the two covers of a round by one efficacy scale is not built")
        if strat not in (1, 2, 4, 5) and not (self._gpu_exact_sdp and strat == 3):      # cut_select_qcqp.py:26 allows 3
            raise AssertionError("strategies on the GPU path: 1 feasibility, 2 optimality, 4 combined, 5 random (3 exact optimality with exact_sdp=True)")
        assert 0 < sel_size, "The selection size must be a % or number (of cuts) >0!"
        assert dim <= 5, "Keep SDP vertex cover low-dimensional (<=5)!"
        m_cuts, _ = _capi.check_multi_args(cuts_per_set, 1)
        inst = harness.parse_osil(filename)
        self._dim = dim
        self._nb_vars, self._nb_lifted, self._Q_arr = inst["nb_vars"], inst["nb_lifted"], inst["Q_arr"]
        self._Q_adj, self._Q_adj_cons = inst["adj"], inst["adj_cons"]
        self._my_prob = lp = harness.LinearRelaxation(np.concatenate([inst["Q_arr"], inst["c"]]))
        lp.linear_constraints.add(inst["rows"], inst["rhs"], inst["senses"])
        lp.linear_constraints.add_csr(*harness.mccormick_csr(self._nb_vars, inst["adj"]), "L")
        self._load_neural_nets()
        # both covers and their intersection on the device (:50, :314-334): the lists never come to the host
        sc_o, sc_c = self._gpu_new_scorer(), self._gpu_new_scorer()
        for sc in (sc_o, sc_c):
            sc.set_instance(self._nb_vars, np.asarray(self._Q_arr, dtype=np.float64))
        n_o, n_c = sc_o.set_candidates_cover_split(sc_c, inst["adj"], inst["adj_cons"], dim)
        cover_obj = DeviceAgg(sc_o, n_o, self._nb_vars, self._Q_arr)
        cover_cons = DeviceAgg(sc_c, n_c, self._nb_vars, self._Q_arr)
        if strat == 5:
            cover_obj = cover_obj.to_arrays()       # the random strategy reorders its list in place, round after round (:634-637)
        self._agg_list = cover_obj
        quota = self.selection_size(sel_size, len(cover_obj), minimum=1)                         # :55-58
        self._run = SimpleNamespace(strat=strat, quota=quota, covers=(cover_obj, cover_cons))
        keep_attr = (self.cuts_per_set, self.cuts_row_quota)
        if m_cuts > 1:
            self.cuts_per_set, self.cuts_row_quota, self.multi_log = m_cuts, None, []
        try:
            log = harness.run_cut_rounds(lp, self._round_qcqp, nb_rounds_cuts, after_solve=self._gpu_wake)
        finally:
            self.cuts_per_set, self.cuts_row_quota = keep_attr
        opt = log.column("opt")
        return log.bounds, quota, [0] + log.column("sdp"), [0] + opt + [0] * (nb_rounds_cuts - len(opt))


def make_dropin_classes(cut_select_qp, cut_select_qcqp=None, exact_heads=False, exact_sdp=False, cuts_per_set=1):
    """Compose the GPU mixin with the reference's own classes (modules passed in, nothing is
    imported here) -> (GpuCutSolver, GpuCutSolverQCQP or None).

    The QCQP loop reaches the hot path through ``super()`` from inside ``CutSolverQCQP``
    (cut_select_qcqp.py:41, :66-76), i.e. through whatever FOLLOWS ``CutSolverQCQP`` in the
    instance's MRO.  Putting the mixin in front of ``CutSolverQCQP`` would leave those calls on
    the reference's CPU loop; the mixin has to sit between the two reference classes:

        GpuCutSolver     = (GpuCutSelectionMixin, CutSolver)
        GpuCutSolverQCQP = (CutSolverQCQP, GpuCutSolver)
        MRO: GpuCutSolverQCQP, CutSolverQCQP, GpuCutSolver, GpuCutSelectionMixin, CutSolver, object

    exact_heads: the classes' ``_gpu_exact_heads`` (SDPCUT_OPT_EXACT_HEAD on every handle they create).
    exact_sdp: the classes' ``_gpu_exact_sdp`` (strategies 3 and -1 on the device instead of a NotImplementedError).
    cuts_per_set: the classes' ``cuts_per_set`` (1 .. 5): ``_gen_eigcuts_selected`` emits up to that many eigen-cuts per selected set
        and keeps the first ``sel_size`` rows (all violated eigen-cuts).
    """
    m_cuts, _ = _capi.check_multi_args(cuts_per_set, 1)
    qp = type("GpuCutSolver", (GpuCutSelectionMixin, cut_select_qp.CutSolver),
              {"__doc__": "CutSolver with the hot path on the GPU", "_gpu_exact_heads": bool(exact_heads), "_gpu_exact_sdp": bool(exact_sdp),
               "cuts_per_set": m_cuts})
    qcqp = None
    if cut_select_qcqp is not None:
        qcqp = type("GpuCutSolverQCQP", (cut_select_qcqp.CutSolverQCQP, qp), {"__doc__": "CutSolverQCQP with the hot path on the GPU"})
    return qp, qcqp
