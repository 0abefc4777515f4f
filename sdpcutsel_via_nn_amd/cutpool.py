"""Cut pool: the numpy twin of csrc/pool.hip and the invariant checker of a step.

The rule ("Cut pool"; include/sdpcut.h: sdpcut_pool_*).  The pool holds the rows a cutting-plane loop has
added, each in the LP (state 0) or parked (state 1), in ascending order of a serial given at add time.  At an LP point ``v``::

    act  = sum over the row's entries, left to right, of value * v[column]     multiply and add separate
    norm = sqrt(sum of value^2), same order, once at add time
    d    = sense * (act - rhs)                                                 d >= 0: satisfied
    in the LP       age = age + 1 if d > tight_tol * norm else 0; parked with age 0 at age >= max_age          -> leave
    parked before   violated iff -d > viol_tol * norm, key (-d) / norm; by (key descending, serial ascending) the first
    the step        max_return return with age 0                                                                -> enter
                    every other parked row: age + 1, dropped at age >= drop_age                                 -> dropped

:class:`CutPoolTwin` restates the device's arithmetic operation by operation (Python floats where the order of a sum matters), so
the two agree bit for bit; it has the methods of ``Scorer.pool_*`` and serves loops that run without a device.
:func:`check_step` checks the invariants of one step from the outside, with its own arithmetic.

The pool at tree nodes (include/sdpcut.h: sdpcut_pool_separate_points, sdpcut_pool_drop).  ``pool_separate_points`` asks which rows P
LP points violate and changes nothing: row r is examined iff ``(1 << state[r]) & state_mask`` ("all" = 3, "lp" = 1, "parked" = 2), an
examined row is violated iff ``-d > viol_tol * norm`` with the key ``(-d) / norm`` -- the step's test and key of a parked row -- and
a point gets its count and the first ``max_return`` violated rows by (key descending, serial ascending).  ``pool_drop`` removes rows
by serial with the step's stable compaction.  :func:`check_separation` checks a separation's invariants from the outside.  :class:`PoolLoop` is the pool's
side of a cutting-plane loop (``CutSolver.cut_select_algo(pool_max_age=...)``): it moves rows between the LP and either pool.
"""
import math
from timeit import default_timer

import numpy as np

from ._capi import POOL_MAX_ROWS, ROW_LD, check_pool_params, check_pool_rows, check_pool_sep_args, check_pool_serials

_STATE_FIELDS = ("serial", "state", "age", "nnz", "sense", "rhs", "norm", "cols", "vals")


def row_distance(cols, vals, nnz, rhs, sense, point):
    """d = sense * (act - rhs) with act summed left to right over the first nnz slots, as the device sums it"""
    act = 0.0
    for s in range(int(nnz)):
        act = act + float(vals[s]) * float(point[int(cols[s])])
    return float(sense) * (act - float(rhs))


def row_norm(vals, nnz):
    ss = 0.0
    for s in range(int(nnz)):
        v = float(vals[s])
        ss = ss + v * v
    return math.sqrt(ss)


def _key(d, norm):
    return float(np.float64(-d) / np.float64(norm)) if norm != 0.0 else (math.inf if -d > 0.0 else math.nan)


class CutPoolTwin(object):
    """The pool on the host: ``pool_add``, ``pool_step`` and ``pool_state`` as :class:`Scorer` has them."""

    def __init__(self, capacity, ncols):
        capacity = int(capacity)
        if not 1 <= capacity <= POOL_MAX_ROWS:
            raise ValueError("capacity must lie in 1 .. %d" % POOL_MAX_ROWS)
        self.pool_capacity, self.ncols = capacity, int(ncols)
        self.next_serial = 0
        self.serial = np.zeros(0, np.int64)
        self.state = np.zeros(0, np.int32)
        self.age = np.zeros(0, np.int32)
        self.nnz = np.zeros(0, np.int32)
        self.sense = np.zeros(0, np.int32)
        self.rhs = np.zeros(0)
        self.norm = np.zeros(0)
        self.cols = np.zeros((0, ROW_LD), np.int32)
        self.vals = np.zeros((0, ROW_LD))
        self._point = None

    @property
    def n(self):
        return int(self.serial.shape[0])

    def pool_add(self, indptr, indices, values, rhs, sense=None):
        indptr, indices, values, rhs, sense = check_pool_rows(indptr, indices, values, rhs, sense, self.ncols,
                                                              self.pool_capacity - self.n)
        m = rhs.shape[0]
        first = self.next_serial
        if m == 0:
            return first
        cols = np.zeros((m, ROW_LD), np.int32)
        vals = np.zeros((m, ROW_LD))
        lens = np.diff(indptr).astype(np.int32)
        norm = np.zeros(m)
        for i in range(m):
            lo, ln = int(indptr[i]), int(lens[i])
            cols[i, :ln] = indices[lo:lo + ln]
            vals[i, :ln] = values[lo:lo + ln]
            norm[i] = row_norm(vals[i], ln)
        self.serial = np.concatenate([self.serial, first + np.arange(m, dtype=np.int64)])
        self.state = np.concatenate([self.state, np.zeros(m, np.int32)])
        self.age = np.concatenate([self.age, np.zeros(m, np.int32)])
        self.nnz = np.concatenate([self.nnz, lens])
        self.sense = np.concatenate([self.sense, sense])
        self.rhs = np.concatenate([self.rhs, rhs])
        self.norm = np.concatenate([self.norm, norm])
        self.cols = np.concatenate([self.cols, cols])
        self.vals = np.concatenate([self.vals, vals])
        self.next_serial += m
        return first

    def pool_step(self, point=None, tight_tol=1e-9, viol_tol=1e-6, max_age=3, drop_age=10, max_return=0, copy=True):
        tt, vt, ma, da, mr = check_pool_params(tight_tol, viol_tol, max_age, drop_age, max_return)
        if point is not None:
            p = np.ascontiguousarray(point, dtype=np.float64)
            if p.shape != (self.ncols,):
                raise ValueError("the point must have one entry per LP column")
            self._point = p
        if self._point is None:
            raise RuntimeError("a point first")
        v = self._point
        n = self.n
        leave, viol = [], []
        parked_before = self.state == 1
        for r in range(n):
            d = row_distance(self.cols[r], self.vals[r], self.nnz[r], self.rhs[r], self.sense[r], v)
            nr = float(self.norm[r])
            if not parked_before[r]:
                g = int(self.age[r]) + 1 if d > tt * nr else 0
                if g >= ma:
                    self.state[r], self.age[r] = 1, 0
                    leave.append(r)
                else:
                    self.age[r] = g
            elif -d > vt * nr:
                viol.append((-_key(d, nr), r))      # key descending, row (= serial) ascending
        viol.sort()
        take = [r for _, r in viol[:mr]]
        keys = [-k for k, _ in viol[:mr]]
        entering = np.zeros(n, bool)
        entering[take] = True
        self.state[take] = 0
        self.age[take] = 0
        rest = parked_before & ~entering
        self.age[rest] += 1
        drop = rest & (self.age >= da)
        out = dict(leave=self.serial[leave].copy(), enter=self.serial[take].copy(), dropped=self.serial[drop].copy())
        lens = self.nnz[take].astype(np.int64)
        out["enter_indptr"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        out["enter_indices"] = (np.concatenate([self.cols[r, :self.nnz[r]] for r in take]) if take else np.zeros(0)).astype(np.int32)
        out["enter_values"] = (np.concatenate([self.vals[r, :self.nnz[r]] for r in take]) if take else np.zeros(0)).astype(np.float64)
        out["enter_rhs"] = self.rhs[take].copy()
        out["enter_sense"] = self.sense[take].copy()
        out["enter_key"] = np.array(keys, dtype=np.float64)
        keep = ~drop
        for f in _STATE_FIELDS:
            setattr(self, f, getattr(self, f)[keep])
        out.update(n_in_lp=int(np.sum(self.state == 0)), n_parked=int(np.sum(self.state == 1)), n_violated=len(viol),
                   n_dropped=int(drop.sum()))
        return out

    def pool_separate_points(self, points, max_return, viol_tol=1e-6, states="all", copy=False):
        """``Scorer.pool_separate_points`` on the host, bit for bit (without ``select_passes``, which describes the kernel)."""
        pts = np.asarray(points, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != self.ncols:
            raise ValueError("points must be [P, n(n+1)/2 + n]: one LP point [X packed | x] per row")
        n = self.n
        mr, vt, mask = check_pool_sep_args(pts.shape[0], max_return, viol_tol, states, n)
        examined = [r for r in range(n) if (1 << int(self.state[r])) & mask]
        res = []
        for v in pts:
            viol = []
            for r in examined:
                d = row_distance(self.cols[r], self.vals[r], self.nnz[r], self.rhs[r], self.sense[r], v)
                nr = float(self.norm[r])
                if -d > vt * nr:
                    viol.append((-_key(d, nr), r))      # key descending, row (= serial) ascending
            viol.sort()
            take = [r for _, r in viol[:mr]]
            lens = self.nnz[take].astype(np.int64)
            res.append(dict(
                serial=self.serial[take].copy(), key=np.array([-k for k, _ in viol[:mr]], dtype=np.float64),
                indptr=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32),
                indices=(np.concatenate([self.cols[r, :self.nnz[r]] for r in take]) if take else np.zeros(0)).astype(np.int32),
                values=(np.concatenate([self.vals[r, :self.nnz[r]] for r in take]) if take else np.zeros(0)).astype(np.float64),
                rhs=self.rhs[take].copy(), sense=self.sense[take].copy(), n_violated=len(viol)))
        return res

    def pool_drop(self, serials):
        ser = check_pool_serials(serials)
        keep = ~np.isin(self.serial, ser)
        gone = int(self.n - keep.sum())
        for f in _STATE_FIELDS:
            setattr(self, f, getattr(self, f)[keep])
        return gone

    def pool_state(self):
        a = {f: getattr(self, f).copy() for f in _STATE_FIELDS}
        a.update(n=self.n, next_serial=self.next_serial)
        return a


class PoolLoop(object):
    """The pool's side of a cutting-plane loop: keeps ``serial of LP row`` (-1 for model rows, which are never pooled) and moves
    rows between the LP and the pool.  ``lp``: a :class:`harness.LinearRelaxation` (``linear_constraints.add_csr``,
    ``delete_rows``); ``pool``: a ``Scorer`` with a pool or a :class:`CutPoolTwin`.  Per round: :meth:`step` at the LP point, the
    separation (which adds its rows to the LP as it always did), :meth:`adopt` for the rows it added."""

    def __init__(self, lp, pool, max_age, drop_age=10, tight_tol=1e-9, viol_tol=1e-6):
        self.lp, self.pool = lp, pool
        self.params = dict(zip(("tight_tol", "viol_tol", "max_age", "drop_age", "max_return"),
                               check_pool_params(tight_tol, viol_tol, max_age, drop_age, 0)))
        self.row_serial = np.full(lp.linear_constraints.get_num(), -1, dtype=np.int64)
        self.log = []
        self.steps = []          # (LP point, dict(leave, enter, dropped)) of every step: what a checker or a tool recomputes from

    def step(self, point, max_return):
        """One pool step at ``point``: the leaving rows are deleted from the LP, the entering ones appended to it (they do
        not count against the round's quota) -> the step's dict."""
        par = dict(self.params, max_return=int(max_return))
        rows_at_solve = int(self.row_serial.shape[0])
        t = default_timer()
        out = self.pool.pool_step(point, **par)
        step_ms = 1e3 * (default_timer() - t)      # host to host: upload of the point, the step's kernels, the one wait
        if out["leave"].size:
            pos = np.flatnonzero(np.isin(self.row_serial, out["leave"]))
            assert pos.size == out["leave"].size, "a leaving row is not in the LP"
            self.lp.delete_rows(pos)
            self.row_serial = np.delete(self.row_serial, pos)
        store = self.lp.linear_constraints
        w = int(out["enter"].shape[0])
        ip = out["enter_indptr"]
        for sense, name in ((1, "G"), (-1, "L")):      # (a block of the row store has one sense)
            sel = np.flatnonzero(out["enter_sense"] == sense)
            if sel.size == 0:
                continue
            if sel.size == w:
                ptr, ind, val = ip, out["enter_indices"], out["enter_values"]
            else:
                lens = np.diff(ip)[sel]
                take = np.concatenate([np.arange(ip[r], ip[r + 1]) for r in sel])
                ptr = np.concatenate([[0], np.cumsum(lens)])
                ind, val = out["enter_indices"][take], out["enter_values"][take]
            store.add_csr(np.array(ptr, dtype=np.int64), np.array(ind), np.array(val), np.array(out["enter_rhs"][sel]), name)
            self.row_serial = np.concatenate([self.row_serial, out["enter"][sel]])
        self.steps.append((np.array(point, dtype=np.float64), {k: out[k].copy() for k in ("leave", "enter", "dropped")}))
        self.log.append(dict(leave=int(out["leave"].size), enter=w, dropped=int(out["dropped"].size), in_lp=out["n_in_lp"],
                             parked=out["n_parked"], violated=out["n_violated"], lp_rows=rows_at_solve, added=0, step_ms=step_ms))
        return out

    def adopt(self):
        """The rows the separation appended to the LP since :meth:`step` enter the pool (in the LP, age 0) -> their number."""
        store = self.lp.linear_constraints
        first, n = int(self.row_serial.shape[0]), store.get_num()
        if n == first:
            return 0
        data, cols, lens = store.csr_parts(first)
        senses = store.senses_from(first)
        if np.any(senses == "E"):
            raise ValueError("equality rows cannot be pooled")
        ptr = np.concatenate([[0], np.cumsum(lens)])
        s0 = self.pool.pool_add(ptr, cols, data, store.rhs_from(first), np.where(senses == "L", -1, 1).astype(np.int32))
        self.row_serial = np.concatenate([self.row_serial, s0 + np.arange(n - first, dtype=np.int64)])
        self.log[-1]["added"] = n - first
        return n - first


def check_step(before, params, point, out, after):
    """Invariants of one pool step, recomputed independently (numpy dot products: another summation order, so a violation or a
    key within 1e-12 relative of its threshold is not judged).

    before / after: ``pool_state()`` around the step (rows added between two steps belong to ``before``); params:
    dict(tight_tol, viol_tol, max_age, drop_age, max_return); out: what ``pool_step`` returned.  Raises AssertionError."""
    vt, mr = float(params["viol_tol"]), int(params["max_return"])
    ma, da = int(params["max_age"]), int(params["drop_age"])
    point = np.asarray(point, dtype=np.float64)
    sb, sa = before["serial"], after["serial"]
    assert np.all(np.diff(sb) > 0) and np.all(np.diff(sa) > 0), "serials must ascend"
    assert after["next_serial"] == before["next_serial"]
    assert sa.size == 0 or sa.max() < after["next_serial"]
    leave, enter, dropped = out["leave"], out["enter"], out["dropped"]
    # every serial of before is in exactly one of in-LP / parked / dropped afterwards
    assert np.array_equal(np.sort(np.concatenate([sa, dropped])), sb), "rows lost or invented"
    assert np.all(np.diff(leave) > 0) and np.all(np.diff(dropped) > 0)
    pos_b = {int(s): i for i, s in enumerate(sb)}
    pos_a = {int(s): i for i, s in enumerate(sa)}
    in_lp_b = set(int(s) for s in sb[before["state"] == 0])
    parked_b = set(int(s) for s in sb[before["state"] == 1])
    assert set(int(s) for s in leave) <= in_lp_b, "a leaving row was not in the LP"
    assert set(int(s) for s in enter) <= parked_b, "an entering row was not parked"
    assert set(int(s) for s in dropped) <= parked_b - set(int(s) for s in enter), "a dropped row was not parked"
    assert len(set(int(s) for s in enter)) == len(enter) <= mr
    assert out["n_in_lp"] == int(np.sum(after["state"] == 0)) and out["n_parked"] == int(np.sum(after["state"] == 1))
    assert out["n_dropped"] == len(dropped) and out["n_violated"] >= len(enter)
    assert len(enter) == min(mr, out["n_violated"])

    def dist(i):
        ln = int(before["nnz"][i])
        act = float(np.dot(before["vals"][i, :ln], point[before["cols"][i, :ln]]))
        return float(before["sense"][i]) * (act - float(before["rhs"][i]))
    # the rows themselves never change
    for s, i in pos_a.items():
        j = pos_b[s]
        for f in ("nnz", "sense", "rhs", "norm"):
            assert after[f][i] == before[f][j]
        assert np.array_equal(after["cols"][i], before["cols"][j]) and np.array_equal(after["vals"][i], before["vals"][j])
    # states and ages afterwards
    for s in leave:
        i = pos_a[int(s)]
        assert after["state"][i] == 1 and after["age"][i] == 0
    for s in in_lp_b - set(int(x) for x in leave):
        i = pos_a[s]
        assert after["state"][i] == 0 and after["age"][i] < ma
        assert after["age"][i] in (0, before["age"][pos_b[s]] + 1)
    for s in enter:
        i = pos_a[int(s)]
        assert after["state"][i] == 0 and after["age"][i] == 0
    for s in parked_b - set(int(x) for x in enter) - set(int(x) for x in dropped):
        i = pos_a[s]
        assert after["state"][i] == 1 and after["age"][i] == before["age"][pos_b[s]] + 1 < da
    for s in dropped:
        assert before["age"][pos_b[int(s)]] + 1 >= da
    # entering rows: violated by more than viol_tol, in (key descending, serial ascending) order, their rows as stored
    keys = np.asarray(out["enter_key"], dtype=np.float64)
    ip = out["enter_indptr"]
    for t, s in enumerate(enter):
        j = pos_b[int(s)]
        d, nr = dist(j), float(before["norm"][j])
        assert -d > vt * nr * (1.0 - 1e-12) - 1e-300, "an entering row is not violated"
        assert nr == 0.0 or abs(keys[t] - (-d) / nr) <= 1e-12 * max(1.0, abs(keys[t])), "key of an entering row"
        ln = int(before["nnz"][j])
        assert ip[t + 1] - ip[t] == ln
        assert np.array_equal(out["enter_indices"][ip[t]:ip[t + 1]], before["cols"][j, :ln])
        assert np.array_equal(out["enter_values"][ip[t]:ip[t + 1]], before["vals"][j, :ln])
        assert out["enter_rhs"][t] == before["rhs"][j] and out["enter_sense"][t] == before["sense"][j]
    for t in range(1, len(enter)):
        assert keys[t - 1] > keys[t] or (keys[t - 1] == keys[t] and enter[t - 1] < enter[t]), "enter is not in rank order"
    # no parked row left out beats the last one taken (beyond the rounding of an independently summed key)
    if len(enter):
        last = keys[-1]
        for s in parked_b - set(int(x) for x in enter):
            j = pos_b[s]
            d, nr = dist(j), float(before["norm"][j])
            if nr > 0.0 and -d > vt * nr * (1.0 + 1e-12) + 1e-300:
                assert (-d) / nr <= last + 1e-12 * max(1.0, abs(last)), "a parked row left out beats the last one taken"
    return True


def check_separation(state, points, viol_tol, states, max_return, out):
    """Invariants of one ``pool_separate_points`` call, recomputed independently (numpy dot products: another summation order, so a
    violation or a key within 1e-12 relative of its threshold is not judged).

    state: ``pool_state()`` at the call; points [P, ncols]; out: the list the call returned.  Checks that every returned row is
    examined and violated, that keys do not increase and equal keys ascend in serial, that no examined row left out beats the last
    one returned, the counts, and that the CSR equals the stored row.  Raises AssertionError."""
    mr, vt, mask = check_pool_sep_args(len(out), max_return, viol_tol, states, state["n"])
    points = np.asarray(points, dtype=np.float64)
    assert points.shape[0] == len(out)
    ser = state["serial"]
    assert np.all(np.diff(ser) > 0), "serials must ascend"
    pos = {int(s): i for i, s in enumerate(ser)}
    examined = ((1 << state["state"].astype(np.int64)) & mask) != 0
    n = int(state["n"])
    # d and the key of every row at every point, by numpy: rows padded with zero values contribute nothing
    lens = state["nnz"]
    live = np.arange(state["cols"].shape[1])[None, :] < lens[:, None]
    vals = np.where(live, state["vals"], 0.0)
    for v, o in zip(points, out):
        act = np.sum(vals * np.where(live, v[state["cols"]], 0.0), axis=1) if n else np.zeros(0)
        d = state["sense"] * (act - state["rhs"])
        nr = state["norm"]
        surely = examined & (-d > vt * nr * (1.0 + 1e-12) + 1e-300)
        maybe = examined & (-d > vt * nr * (1.0 - 1e-12) - 1e-300)
        assert int(surely.sum()) <= o["n_violated"] <= int(maybe.sum()), "n_violated"
        w = int(o["serial"].shape[0])
        assert w == min(mr, o["n_violated"]), "the number of returned rows"
        keys, ip = np.asarray(o["key"], dtype=np.float64), o["indptr"]
        assert keys.shape == (w,) and ip.shape == (w + 1,) and ip[0] == 0
        assert o["rhs"].shape == (w,) and o["sense"].shape == (w,)
        assert o["indices"].shape == o["values"].shape == (int(ip[-1]),)
        assert len(set(int(s) for s in o["serial"])) == w, "a row returned twice"
        taken = np.zeros(n, bool)
        for t, s in enumerate(o["serial"]):
            assert int(s) in pos, "a returned serial is not in the pool"
            j = pos[int(s)]
            taken[j] = True
            assert examined[j], "a returned row was not examined"
            assert maybe[j], "a returned row is not violated"
            if nr[j] > 0.0:
                assert abs(keys[t] - (-d[j]) / nr[j]) <= 1e-12 * max(1.0, abs(keys[t])), "key of a returned row"
            else:
                assert keys[t] == math.inf, "key of a zero-norm row"
            ln = int(lens[j])
            assert ip[t + 1] - ip[t] == ln
            assert np.array_equal(o["indices"][ip[t]:ip[t + 1]], state["cols"][j, :ln])
            assert np.array_equal(o["values"][ip[t]:ip[t + 1]], state["vals"][j, :ln])
            assert o["rhs"][t] == state["rhs"][j] and o["sense"][t] == state["sense"][j]
        for t in range(1, w):
            assert keys[t - 1] > keys[t] or (keys[t - 1] == keys[t] and o["serial"][t - 1] < o["serial"][t]), "not in rank order"
        if w:
            last = keys[-1]
            rest = surely & ~taken & (nr > 0.0)
            if rest.any():
                assert np.max(-d[rest] / nr[rest]) <= last + 1e-12 * max(1.0, abs(last)), "a row left out beats the last one returned"
            assert not np.any(surely & ~taken & (nr == 0.0)) or last == math.inf, "a zero-norm row left out beats the last one returned"
    return True
