"""Containers of the host layer above the C-ABI: the lazy rank lists the cutting-plane loop slices and concatenates, the
device-side twin of a candidate list, the array-backed candidate lists, and the two array helpers they share with the cut
generation (padded rows -> CSR, the CSR prefix of a round's first entries).  Nothing here knows the mixin of cut_solver.py."""
from collections.abc import Sequence

import numpy as np

_BIG_M = 1000                         # cut_select_qp.py:26


def packed_positions(s, n):
    """Positions of X_ab, a <= b in s, in the packed upper triangle of the n x n lifted matrix: ``Xarr_inds`` of the index set
    ``s`` (cut_select_qp.py:533)."""
    k = len(s)
    return [n * s[a] - s[a] * (s[a] + 1) // 2 + s[b] for a in range(k) for b in range(a, k)]


def packed_positions_rows(S, n):
    """:func:`packed_positions` of every row of the int64 array ``S`` [m, k] at once -> [m, k(k+1)/2]"""
    ia, ib = np.triu_indices(S.shape[1])
    A = S[:, ia]
    return n * A - A * (A + 1) // 2 + S[:, ib]


def rows_to_csr(coef, cols, ks):
    """Padded cut rows (stride SDPCUT_ROW_LD, row c has k_c(k_c+3)/2 live entries) -> CSR
    (indptr int64 [R+1], indices int64, values float64)."""
    ks = np.asarray(ks, dtype=np.int64)
    lens = ks * (ks + 3) // 2
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    live = np.arange(coef.shape[1])[None, :] < lens[:, None]
    return indptr, np.ascontiguousarray(cols[live], dtype=np.int64), np.ascontiguousarray(coef[live], dtype=np.float64)


def strong_prefix(scores, count):
    """``count`` cut down to the entries before the first score <= 0 (cut_select_qp.py:725-726)"""
    stop = np.flatnonzero(scores[:count] <= 0)
    return int(stop[0]) if stop.size else count


def csr_prefix(r, count):
    """The assembled cuts that belong to the first ``count`` entries of a round dict (Scorer.round_csr and its kin) as
    (indptr, indices, values, rhs) views: ``row_entry`` ascends, so they are a prefix of the block."""
    rows = int(np.searchsorted(r["row_entry"], count))
    nnz = int(r["indptr"][rows])
    return r["indptr"][:rows + 1], r["indices"][:nnz], r["values"][:nnz], r["rhs"][:rows]


class FeasEntry(tuple):
    """``(set_inds, -eigval, Xarr_inds, dim_act)`` of cut_select_qp.py:649, remembering which
    candidate it came from so that cut generation needs no search."""
    agg_idx = -1
    binding = None

    def __new__(cls, items, agg_idx, binding=None):
        self = super().__new__(cls, items)
        self.agg_idx = agg_idx
        self.binding = binding
        return self


class RankList(Sequence):
    """Lazy stand-in for the reference's sorted ``rank_list``.

    The reference materialises N Python tuples; downstream code only looks at the first
    ``sel_size`` of them.  This object keeps the ranking on the device, fetches windows on
    demand (``sdpcut_rank_fetch``) and builds entry tuples only for what is indexed.
    ``a + b`` (cut_select_qcqp.py:79) and slicing return plain lists of entries.
    """

    def __init__(self, binding, kind, total, vars_values, head_idx, head_score, strat=None, sel_size=0, fused=None):
        self._b, self._kind, self._n = binding, kind, int(total)
        self._vv = vars_values
        self._strat, self._sel_size = strat, sel_size
        self._idx, self._score = head_idx, head_score
        self._have = head_idx.shape[0]
        self._point = binding.point_token
        # fused round (sdpcut_round_csr): the cuts of the head already sit, assembled, in the scorer's pinned block;
        # `fused` holds views of it, good until the scorer runs its next round (round_count moves on)
        self._fused, self._fused_at = fused, binding.scorer.round_count
        self._head_sets = self._head_ks = None
        if fused is not None:
            self._head_sets, self._head_ks = fused["set_inds"].copy(), fused["ks"].copy()

    def fused_rows(self, count, strong_only=False, vars_values=None):
        """The assembled cuts of the first ``count`` entries if the fused round's block still holds them:
        (indptr, indices, values, rhs) views, or None (stale block, longer head, another LP point)."""
        f = self._fused
        if f is None or self._b.scorer.round_count != self._fused_at or count > self._have:
            return None
        if vars_values is not None and vars_values is not self._vv and not np.array_equal(vars_values, self._vv):
            return None
        return csr_prefix(f, strong_prefix(self._score, count) if strong_only else count)

    # -- data access -----------------------------------------------------------------
    def _need(self, upto):
        """The head came from the device's top-k selection; anything beyond it asks for the
        complete ranking (full device sort), once."""
        upto = min(upto, self._n)
        if upto <= self._have:
            return
        if self._b.point_token != self._point:
            raise RuntimeError("rank list is stale: the device now holds the scores of a newer LP point")
        self._b.drain()
        idx, sc, total, _, _ = self._b.scorer.rank(self._strat, self._sel_size, max_out=self._n)
        self._idx, self._score, self._have = idx, sc, idx.shape[0]

    def ids(self, count=None):
        count = self._n if count is None else min(count, self._n)
        self._need(count)
        return self._idx[:count]

    def scores(self, count=None):
        count = self._n if count is None else min(count, self._n)
        self._need(count)
        return self._score[:count]

    def count_above(self, thr):
        """Number of entries of the WHOLE list whose score exceeds ``thr`` (cut_select_qcqp.py:85-87 counts the entries above
        BIG_M).  The list is sorted by score, so the head answers when its last score is <= thr; under the combined strategy a
        head that consists of marked entries only (obj_improve + BIG_M, cut_select_qp.py:611) answers too when the entries behind
        it -- the ones the scan never reached, all with an obj_improve no larger than the last marked one's -- cannot exceed thr.
        Otherwise the complete ranking is fetched."""
        h = self._score
        if self._have == 0:
            return 0
        last = float(h[self._have - 1])
        if self._have >= self._n or last <= thr or (self._strat == 4 and last > _BIG_M and last - _BIG_M <= thr):
            return int(np.count_nonzero(h[:self._have] > thr))
        return int(np.count_nonzero(self.scores() > thr))

    def _sets(self, lo, hi, loc):
        """(index sets [m, 5], sizes [m]) of positions [lo, hi): from the fused round's head when it covers them"""
        if self._head_sets is not None and hi <= self._head_sets.shape[0]:
            return self._head_sets[lo:hi], self._head_ks[lo:hi]
        return self._b.sets_of(loc)

    def _entry(self, pos):
        idx, score = int(self._idx[pos]), float(self._score[pos])
        if self._b.agg_list is None or isinstance(self._b.agg_list, DeviceAgg):
            S, ks = self._sets(pos, pos + 1, np.array([idx - self._b.scorer.base], dtype=np.int64))
            set_inds = [int(v) for v in S[0, :int(ks[0])]]
            Xarr_inds = packed_positions(set_inds, self._b.nb_vars)
        else:
            set_inds, Xarr_inds = self._b.agg_entry(idx)
        if self._kind == 1:
            return FeasEntry((set_inds, score, Xarr_inds, len(set_inds)), idx, self._b)
        L = self._b.nb_lifted
        curr_pt = tuple(self._vv[L + i] for i in set_inds)
        X_slice = tuple(self._vv[i] for i in Xarr_inds)
        return (idx, score, curr_pt, X_slice)

    def _entries(self, lo, hi):
        """Entry tuples of positions [lo, hi) built with array gathers (one fancy-indexing pass per
        candidate size instead of a Python loop per value): what iteration and slicing use."""
        hi = min(hi, self._n)
        if hi <= lo:
            return []
        if hi - lo < 8:
            return [self._entry(p) for p in range(lo, hi)]
        b, vv, L, n = self._b, self._vv, self._b.nb_lifted, self._b.nb_vars
        ids = np.asarray(self._idx[lo:hi], dtype=np.int64)
        loc = ids - b.scorer.base
        scores = np.asarray(self._score[lo:hi], dtype=np.float64).tolist()
        S_all, ks = self._sets(lo, hi, loc)
        out = [None] * (hi - lo)
        for k in np.unique(ks):
            k = int(k)
            m = np.nonzero(ks == k)[0]
            S = S_all[m, :k].astype(np.int64)
            pos = packed_positions_rows(S, n)
            if self._kind == 1:
                for j, s_row, p_row in zip(m.tolist(), S.tolist(), pos.tolist()):
                    i = int(ids[j])
                    if b.agg_list is not None and not isinstance(b.agg_list, DeviceAgg):      # hand out the caller's own lists, as the reference does
                        s_row, p_row = b.agg_list[int(loc[j])][0:2]
                    out[j] = FeasEntry((s_row, scores[j], p_row, k), i, b)
            else:
                cp, Xs = vv[L + S].tolist(), vv[pos].tolist()
                for t, j in enumerate(m.tolist()):
                    out[j] = (int(ids[j]), scores[j], tuple(cp[t]), tuple(Xs[t]))
        return out

    # -- Sequence protocol -----------------------------------------------------------
    def __len__(self):
        return self._n

    def __getitem__(self, key):
        if isinstance(key, slice):
            rng = range(*key.indices(self._n))
            if not len(rng):
                return []
            self._need((rng[-1] if rng.step > 0 else rng[0]) + 1)      # (max(rng) walks the range: 16 us for a head of 5000)
            if rng.step == 1 and rng.start == 0:
                return RankListHead(self, rng.stop)
            if rng.step == 1:
                return self._entries(rng.start, rng.stop)
            return [self._entry(p) for p in rng]
        if key < 0:
            key += self._n
        if not 0 <= key < self._n:
            raise IndexError(key)
        self._need(key + 1)
        return self._entry(key)

    def __iter__(self):
        for lo in range(0, self._n, 65536):
            hi = min(lo + 65536, self._n)
            self._need(hi)
            for e in self._entries(lo, hi):
                yield e

    def __add__(self, other):
        """``a + b`` of cut_select_qcqp.py:79 without building either list: the caller slices
        ``[0:sel_size]`` off the concatenation, and only that slice is materialised."""
        return _Concat([self, other])

    def __radd__(self, other):
        return _Concat([other, self])


class RankListHead(Sequence):
    """``rank_list[0:count]`` (cut_select_qp.py:181 hands the whole list over, cut_select_qcqp.py:79-97 slices of
    it): the entries are built when somebody looks at them, and cut generation still finds the rows the fused
    round assembled for exactly these candidates."""

    def __init__(self, parent, count):
        self.parent, self._n = parent, int(count)
        self._list = None

    def _entries(self):
        if self._list is None:
            self._list = self.parent._entries(0, self._n)
        return self._list

    def __len__(self):
        return self._n

    def __getitem__(self, key):
        if isinstance(key, slice):
            start, stop, step = key.indices(self._n)
            if start == 0 and step == 1:
                return RankListHead(self.parent, stop)
        return self._entries()[key]

    def __iter__(self):
        return iter(self._entries())

    def __eq__(self, other):
        return list(self) == list(other)

    def __add__(self, other):
        return _Concat([self, other])

    def __radd__(self, other):
        return _Concat([other, self])


class _Concat(Sequence):
    """Lazy concatenation of rank lists (``rank_list_comb_obj + rank_list_feas_cons``)."""

    def __init__(self, parts):
        self._parts = [p for p in parts]

    def __len__(self):
        return sum(len(p) for p in self._parts)

    def __iter__(self):
        for p in self._parts:
            for e in p:
                yield e

    def __getitem__(self, key):
        n = len(self)
        if isinstance(key, slice):
            start, stop, step = key.indices(n)
            if step != 1:
                return [self[i] for i in range(start, stop, step)]
            # a slice stays a concatenation of (slices of) its parts: heads of rank lists keep the link to the cuts
            # their fused rounds assembled (cut_select_qcqp.py:79 slices (A + B)[0:sel_size] before generating)
            sub, off = [], 0
            for p in self._parts:
                lo, hi = max(start - off, 0), min(stop - off, len(p))
                if lo < hi:
                    sub.append(p[lo:hi])
                off += len(p)
            return _Concat(sub)
        if key < 0:
            key += n
        off = 0
        for p in self._parts:
            if key - off < len(p):
                return p[key - off]
            off += len(p)
        raise IndexError(key)

    def __eq__(self, other):
        return list(self) == list(other)

    def __add__(self, other):
        return _Concat(self._parts + [other])

    def __radd__(self, other):
        return _Concat([other] + self._parts)


class _Binding(object):
    """Device-side twin of one ``agg_list``: a Scorer handle holding its index sets."""

    def __init__(self, scorer, agg_list, nb_vars, nb_lifted):
        self.scorer, self.agg_list = scorer, agg_list
        self.nb_vars, self.nb_lifted = nb_vars, nb_lifted
        self.rank_serial = 0
        self.point_token = None  # identifies the LP point whose scores the device holds
        self.point_copy = None   # copy of the LP point last uploaded through this binding
        self.point_serial = 0
        self.scored = 0
        self.serial = 0
        self.set_arr = None      # [N, 5] index sets as arrays (vectorised entry building)
        # a fused round begun on the scorer and not yet ended (sdpcut_round_csr_begin): (strat, head, LP point)
        self._pending = None
        # (binding, head) ranked by feasibility right after this one at the same LP point last time (the QCQP round's
        # second cover, cut_select_qcqp.py:75-76): its round is begun together with this one's
        self.follower = None
        self.leader = None       # the binding this one follows (a follower never leads: no cycles)
        self.wasted = 0          # speculative rounds nobody asked for
        self.prioritised = False # its scorer's stream has been given the device's highest priority (a short list beside a long one)

    point_fresh = False          # the cut pool's step has just uploaded the point a round is about to pass (point_arg)

    def point_arg(self, vv):
        """the point argument of a round call: None (keep the device's point) right after a pool step at this very point"""
        fresh, self.point_fresh = self.point_fresh, False
        if fresh and self.point_copy is not None and self.point_copy.shape == vv.shape and np.array_equal(vv, self.point_copy):
            return None
        return vv

    def begin(self, strat, head, vv, flags):
        token = self.scorer.round_csr_begin(strat, head, point=self.point_arg(vv))
        self.note_point(vv, flags)
        self._pending = (token, strat, head, self.point_copy)

    @property
    def pending(self):
        """(strat, head, LP point) of the round begun through this binding and still pending on its scorer, or None"""
        p = self._pending
        if p is not None and self.scorer.pending is not p[0]:       # somebody ended or dropped it on the scorer
            p = self._pending = None
        return None if p is None else p[1:]

    def end(self):
        self._pending = None
        return self.scorer.round_csr_end()

    def drain(self):
        """end a round nobody collected (the scorer's block and scores are about to be used for something else)"""
        if self.pending is not None:
            self.end()
            self.wasted += 1
            if self.leader is not None:                   # the pair is not a pattern after all
                self.leader.follower, self.leader = None, None

    def note_point(self, vv, scored=0):
        """the device now holds LP point ``vv`` (and the measures ``scored`` at it)"""
        self.point_serial += 1
        self.point_token = self.point_serial
        self.point_copy = np.array(vv, dtype=np.float64)
        self.scored = scored

    def agg_entry(self, idx):
        if self.agg_list is not None:
            e = self.agg_list[idx]
            return e[0], e[1]
        S, ks = self.sets_of(np.array([idx], dtype=np.int64))
        s = [int(v) for v in S[0, :int(ks[0])]]
        return s, packed_positions(s, self.nb_vars)

    def sets_of(self, local_ids):
        """(index sets [m, 5], sizes [m]) of candidates by local index: from the host arrays the
        list was bound from, or fetched from the device for lists that only exist there."""
        if self.set_arr is not None:
            return self.set_arr[local_ids], self.ks[local_ids]
        self.drain()
        return self.scorer.get_candidates(local_ids)


class AggArrays(Sequence):
    """Array-backed ``agg_list``: the candidate records of cut_select_qp.py:529-540 built on
    demand.  A Python list of 1.7e6 tuples (spar125-075-1, dim 4) takes minutes to build and
    GBs to hold; the loop only ever reads ``[0]`` / ``[1]`` of the few thousand selected entries."""

    def __init__(self, set_inds, ks, nb_vars, Q_arr=None):
        self.set_inds = np.ascontiguousarray(set_inds, dtype=np.int32)
        self.ks = np.ascontiguousarray(ks, dtype=np.int32)
        self.nb_vars, self.Q_arr = nb_vars, Q_arr
        self.serial = 0          # bumped by shuffle(): device bindings of the old order are stale

    def __len__(self):
        return self.ks.shape[0]

    def shuffle(self):
        """In-place random reordering, the array form of ``np.random.shuffle(agg_list)``
        (cut_select_qp.py:636): ``np.random.permutation(N)`` draws the same permutation from the
        global legacy generator as the list shuffle would (same seed -> same order)."""
        perm = np.random.permutation(len(self))
        self.set_inds = np.ascontiguousarray(self.set_inds[perm])
        self.ks = np.ascontiguousarray(self.ks[perm])
        self.serial += 1

    def __getitem__(self, idx):
        if isinstance(idx, slice):
            return [self[i] for i in range(*idx.indices(len(self)))]
        k = int(self.ks[idx])
        s = [int(v) for v in self.set_inds[idx, :k]]
        pos = packed_positions(s, self.nb_vars)
        if self.Q_arr is None:
            return (s, pos, None, None)
        q = [self.Q_arr[p] for p in pos]
        max_elem = k * abs(max(q, key=abs))
        max_elem += 1 if not max_elem else 0
        return (s, pos, tuple(np.divide(q, max_elem)), max_elem)


class DeviceAgg(Sequence):
    """``agg_list`` whose index sets were enumerated on the device and never came to the host
    (``sdpcut_set_candidates_cover``): a length, and records fetched on demand for the few entries
    somebody indexes.  Bound to the scorer that holds the list."""

    def __init__(self, scorer, count, nb_vars, Q_arr=None):
        self.scorer, self._n, self.nb_vars, self.Q_arr = scorer, int(count), nb_vars, Q_arr
        self.serial = 0

    def __len__(self):
        return self._n

    def __getitem__(self, idx):
        if isinstance(idx, slice):
            rng = range(*idx.indices(self._n))
            S, ks = self.scorer.get_candidates(np.fromiter(rng, dtype=np.int64, count=len(rng)))
            return [AggArrays(S[i:i + 1], ks[i:i + 1], self.nb_vars, self.Q_arr)[0] for i in range(len(rng))]
        if idx < 0:
            idx += self._n
        if not 0 <= idx < self._n:
            raise IndexError(idx)
        S, ks = self.scorer.get_candidates(np.array([idx], dtype=np.int64))
        return AggArrays(S, ks, self.nb_vars, self.Q_arr)[0]

    def to_arrays(self):
        """the whole list on the host (tests; the random strategy reorders a host copy)"""
        S, ks = self.scorer.get_candidates(np.arange(self._n, dtype=np.int64))
        return AggArrays(S, ks, self.nb_vars, self.Q_arr)
