"""Diverse cut selection: the numpy twin of csrc/diverse.hip (sdpcut_round_csr_diverse, sdpcut_filter_parallel).

The rule ("Diverse selection").  A pool of P entries in rank order; entry t has the cut row ``coef[t]`` --
``k + k(k+1)/2`` coefficients on the LP columns ``[L + i for i in set_inds] + Xarr_inds``, what ``Scorer.cut_rows`` returns -- and is
*eligible* iff ``lam_min < -1e-15`` and its row is not zero.  The walk goes through t = 0, 1, ...: an eligible entry is accepted iff
fewer than ``quota`` are accepted so far and every accepted s has ``|<a_s, a_t>| <= max_parallel |a_s| |a_t|``.  The inner product
runs over the shared LP columns: two rows share a column only if their index sets share a variable -- x_c for every common variable
c, X_cd for common c <= d.  ``max_parallel >= 1`` makes no comparison at all.  The walk ends with the entry that fills the quota.

Everything here follows the kernel's arithmetic: coefficient positions ``a`` for x of local index a and ``k + a k - a(a-1)/2 + (b-a)``
for X of the local pair a <= b; sums in a fixed order (x columns by ascending local index of the LATER entry, then the X pairs
row-major); comparison without a division.  The device may still differ from the twin in the last bit of a product
(``undecided_pairs`` lists the pairs where that could matter).
"""
import numpy as np

NEG_EIGVAL = -1e-15      # _THRES_NEG_EIGVAL, cut_select_qp.py:24
ROW_LD = 20


def _arrays(set_inds, ks, coef):
    S = np.asarray(set_inds, dtype=np.int64)
    ks = np.asarray(ks, dtype=np.int64)
    C = np.asarray(coef, dtype=np.float64)
    P = ks.shape[0]
    if S.ndim != 2 or S.shape[0] != P or S.shape[1] > 5 or C.ndim != 2 or C.shape[0] != P:
        raise ValueError("set_inds must be [P, <= 5], ks [P] and coef [P, >= k + k(k+1)/2]")
    if P and (ks.min() < 2 or ks.max() > 5 or S.shape[1] < ks.max() or C.shape[1] < int(ks.max()) * (int(ks.max()) + 3) // 2):
        raise ValueError("candidate sizes must be 2 .. 5 and the arrays wide enough for the largest")
    S5 = np.full((P, 5), -1, dtype=np.int64)
    S5[:, :S.shape[1]] = S
    S5[np.arange(5)[None, :] >= ks[:, None]] = -1
    C20 = np.zeros((P, ROW_LD))
    w = min(C.shape[1], ROW_LD)
    C20[:, :w] = C[:, :w]
    C20[np.arange(ROW_LD)[None, :] >= (ks * (ks + 3) // 2)[:, None]] = 0.0
    return S5, ks, C20


def row_norms(ks, coef):
    """|a_t| of every row: square root of the sum of squares in position order (the kernel's order)"""
    ks = np.asarray(ks, dtype=np.int64)
    C = np.asarray(coef, dtype=np.float64)
    ss = np.zeros(C.shape[0])
    for m in range(min(C.shape[1], ROW_LD)):
        v = np.where(m < ks * (ks + 3) // 2, C[:, m], 0.0)
        ss = ss + v * v
    return np.sqrt(ss)


def _dots_block(St, kt, Ct, Ss, kss, Cs):
    """dots[i, j] = <a_j, a_i> of rows i of the first group (index sets St [nt, 5] padded with -1, sizes kt, rows Ct [nt, 20]) against
    rows j of the second, over their shared LP columns, summed in the order of the FIRST group's local indices"""
    nt, ns = kt.shape[0], kss.shape[0]
    cols = np.arange(ns)[None, :]
    # m[a][i, j] = position in j's set of the a-th variable of i, -1 if not shared
    m = []
    for a in range(5):
        ma = np.full((nt, ns), -1, dtype=np.int64)
        for b in range(5):
            hit = (St[:, a][:, None] >= 0) & (St[:, a][:, None] == Ss[:, b][None, :])
            ma[hit] = b
        m.append(ma)
    acc = np.zeros((nt, ns))
    for a in range(5):
        ok = m[a] >= 0
        acc = acc + np.where(ok, Ct[:, a][:, None] * Cs[cols, np.where(ok, m[a], 0)], 0.0)
    ksr = kss[None, :]
    for a in range(5):
        for b in range(a, 5):
            ok = (m[a] >= 0) & (m[b] >= 0)
            if not ok.any():
                continue
            pa, pb = np.minimum(m[a], m[b]), np.maximum(m[a], m[b])
            pos_s = np.where(ok, ksr + pa * ksr - pa * (pa - 1) // 2 + (pb - pa), 0)
            pos_t = np.where(a < kt, kt + a * kt - a * (a - 1) // 2 + (b - a), 0)
            acc = acc + np.where(ok, Ct[np.arange(nt), pos_t][:, None] * Cs[cols, pos_s], 0.0)
    return acc


def pair_dots(set_inds, ks, coef, chunk=256):
    """-> (dots [P, P], norms [P]): dots[t, s] = <a_s, a_t> over the shared LP columns, summed in the order of the LATER entry t
    (row index); norms as :func:`row_norms`.  Memory: a few [chunk, P] arrays at a time."""
    S5, ks, C = _arrays(set_inds, ks, coef)
    P = ks.shape[0]
    dots = np.zeros((P, P))
    for lo in range(0, P, chunk):
        hi = min(lo + chunk, P)
        dots[lo:hi] = _dots_block(S5[lo:hi], ks[lo:hi], C[lo:hi], S5, ks, C)
    return dots, row_norms(ks, C)


def pair_cosines(set_inds, ks, coef):
    """Cosines of all pairs of rows over their shared LP columns -> [P, P], entry [t, s] = <a_s, a_t> / (|a_s| |a_t|)
    (0 where a row is zero).  The walk itself never divides (:func:`greedy_filter`); this is for inspection and tests."""
    dots, nr = pair_dots(set_inds, ks, coef)
    den = nr[:, None] * nr[None, :]
    out = np.zeros_like(dots)
    np.divide(dots, den, out=out, where=den > 0)
    return out


def eligible_rows(lam_min, ks, coef):
    """eligibility of the rule: lam_min < -1e-15 and a row that is not zero"""
    return (np.asarray(lam_min) < NEG_EIGVAL) & (row_norms(ks, coef) > 0)


def _walk(conflict, eligible, quota):
    """the walk on a conflict matrix (conflict[t, s] for s < t) -> (keep, examined)"""
    P = eligible.shape[0]
    keep = np.zeros(P, dtype=bool)
    acc = []
    examined = 0
    for t in range(P):
        if len(acc) >= quota:
            break
        examined = t + 1
        if not eligible[t]:
            continue
        if conflict is not None and acc and conflict[t, acc].any():
            continue
        keep[t] = True
        acc.append(t)
    return keep, examined


def greedy_filter(set_inds, ks, coef, eligible, quota, max_parallel, return_info=False, dots=None):
    """The walk -> keep bool [P]; with return_info also dict(pool, examined, skipped_nonviolated, rejected_parallel, closest).
    ``closest`` = the smallest | |cos| - max_parallel | over the pairs (accepted s, eligible t > s) -- the only pairs the outcome
    depends on; inf if there is none.
    dots: what :func:`pair_dots` returned for these rows -- or for a longer list these are the first P entries of (an entry of the
    pair matrix depends on its two rows alone) -- to walk several prefixes of one pool without computing it again.  Without it
    only the columns of accepted entries are computed, one per acceptance: O(accepted x P) instead of O(P^2)."""
    eligible = np.asarray(eligible, dtype=bool)
    mp = float(max_parallel)
    if not 0.0 <= mp <= 1.0:
        raise ValueError("max_parallel must lie in [0, 1]")
    quota = int(quota)
    if quota < 1:
        raise ValueError("the quota must be >= 1")
    P = eligible.shape[0]
    closest = np.inf
    if mp >= 1.0:
        keep, examined = _walk(None, eligible, quota)
    else:
        if dots is None:
            S5, kk, C = _arrays(set_inds, ks, coef)
            nr = row_norms(kk, C)
        else:
            full, nr = dots[0], dots[1][:P]
        keep = np.zeros(P, dtype=bool)
        blocked = np.zeros(P, dtype=bool)
        n_acc = examined = 0
        for t in range(P):
            if n_acc >= quota:
                break
            examined = t + 1
            if not eligible[t] or blocked[t]:
                continue
            keep[t] = True
            n_acc += 1
            if t + 1 < P:
                # column t of the pair matrix: every later entry against the newly accepted one, summed in the later entry's order
                col = (_dots_block(S5[t + 1:], kk[t + 1:], C[t + 1:], S5[t:t + 1], kk[t:t + 1], C[t:t + 1])[:, 0] if dots is None
                       else full[t + 1:P, t])
                bound = mp * nr[t] * nr[t + 1:]      # (max_parallel |a_s|) |a_t|, as the kernel multiplies
                blocked[t + 1:] |= np.abs(col) > bound
                den = nr[t] * nr[t + 1:]
                live = eligible[t + 1:] & (den > 0)
                if live.any():
                    closest = min(closest, float(np.abs(np.abs(col[live]) / den[live] - mp).min()))
    if not return_info:
        return keep
    return keep, dict(walk_info(keep, eligible, examined), closest=closest)


def walk_info(keep, eligible, examined):
    seen = np.arange(keep.shape[0]) < examined
    return dict(pool=int(keep.shape[0]), examined=int(examined), skipped_nonviolated=int((seen & ~eligible).sum()),
                rejected_parallel=int((seen & eligible & ~keep).sum()))


def undecided_pairs(set_inds, ks, coef, eligible, max_parallel, margin, cos=None):
    """Pairs (s, t), s < t, of eligible entries whose |cos| lies within ``margin`` of ``max_parallel``: where the device and the
    twin -- or two orders of summation -- may decide differently.  -> int64 [m, 2]."""
    eligible = np.asarray(eligible, dtype=bool)
    P = eligible.shape[0]
    cos = np.abs(pair_cosines(set_inds, ks, coef) if cos is None else cos[:P, :P])      # (cos: a longer list's, as in greedy_filter)
    near = np.abs(cos - float(max_parallel)) <= margin
    near &= eligible[:, None] & eligible[None, :]
    t, s = np.nonzero(np.tril(near, -1))
    return np.stack([s, t], axis=1).astype(np.int64)


def check_walk(set_inds, ks, coef, eligible, quota, max_parallel, keep, margin=0.0, examined=None, cos=None):
    """The invariants of a walk's answer, for answers that cannot be compared bit for bit (tied cosines at a structured vertex):
      * accepted entries are eligible and at most ``quota`` of them;
      * every accepted pair has |cos| <= max_parallel + margin;
      * every eligible entry ranked before the last accepted one and not accepted has an accepted predecessor with
        |cos| >= max_parallel - margin;
      * if fewer than ``quota`` are accepted the whole pool was examined: the same holds for every entry of the pool
        (and ``examined``, if given, equals the pool's length).
    Raises AssertionError naming the first violation; returns True."""
    eligible = np.asarray(eligible, dtype=bool)
    keep = np.asarray(keep, dtype=bool)
    P = eligible.shape[0]
    assert keep.shape == (P,), "keep must have one flag per pool entry"
    acc = np.flatnonzero(keep)
    assert acc.size <= quota, "%d entries accepted, the quota is %d" % (acc.size, quota)
    assert eligible[acc].all(), "entry %d is accepted but not eligible" % (acc[~eligible[acc]][0] if acc.size else -1)
    full = acc.size >= quota
    if not full and examined is not None:
        assert int(examined) == P, "quota not reached but only %d of %d entries examined" % (examined, P)
    if float(max_parallel) >= 1.0:
        # no comparison at all: the first `quota` eligible entries
        want = np.flatnonzero(eligible)[:quota]
        assert np.array_equal(acc, want), "max_parallel >= 1 keeps the first eligible entries"
        return True
    cos = np.abs(pair_cosines(set_inds, ks, coef) if cos is None else cos[:P, :P])
    if acc.size > 1:
        sub = np.tril(cos[np.ix_(acc, acc)], -1)
        i, j = np.unravel_index(np.argmax(sub), sub.shape)
        assert sub[i, j] <= max_parallel + margin, \
            "accepted entries %d and %d have |cos| = %.17g > %g" % (acc[j], acc[i], sub[i, j], max_parallel)
    end = P if not full else (int(acc[-1]) if acc.size else 0)
    for t in np.flatnonzero(eligible & ~keep):
        if t >= end:
            break
        pred = acc[acc < t]
        assert pred.size and cos[t, pred].max() >= max_parallel - margin, \
            "eligible entry %d is rejected without an accepted predecessor that is parallel to it" % t
    return True
