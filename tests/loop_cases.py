"""The cut loop under pairs of options: the option model, the committed combinations, the runner and the row certificate of
test_loop_cases_cpu.py (model, coverage and certificate alone, no GPU) and test_gpu_loop_pairs.py (every committed combination
through ``CutSolver.cut_select_algo`` with every LP row held valid).  A plain module: no fixtures, no GPU at import.

Axes.  ``AXES`` names every option axis with its neutral value and its active values; the strategy is the seventh kind of
choice (``STRATS``; 3 stands for ``CutSolver(exact_sdp=True)`` with ``strat=3``).  A ``Combo`` is one value per axis plus the
cover dimension; ``C(strat, axis=value, ...)`` writes one with everything else neutral.

Model.  ``accepted(combo)`` restates what the docstring of ``cut_select_algo`` documents as refused; it imports none of the
checks.  test_loop_cases_cpu.py holds it against the real entry point over the full product of values.

Committed list.  ``COMMITTED`` is data: ``ALONE`` (every strategy alone and every strategy with one active option value, which
contains every axis alone), ``PAIRS_FEAS`` and ``PAIRS_OPT`` (every unordered pair of active option values once under a strategy of
the family 1 / 5 and once under one of 2 / 4 / 6 -- the two families take different routes through the host layer: strategy 5
through ``_round_plain`` and ``cut_rows_all``, strategies 2, 4 and 6 with their measures and the switch), ``TRIPLES`` (seeded) and
``EVERYTHING`` (per strategy, all that may be on together).  ``uncovered_pairs()`` lists what the coverage test must find empty.

Certificate (``certify``).  A row ``a . v >= rhs`` over ``v = [X packed | x]`` is accepted only in one of two shapes:

* eigen-cut: columns exactly ``L + s_i`` for an index set ``s`` of k = 2..5 variables (or all n) plus the packed positions of all
  pairs of ``s``.  With ``C00 = -rhs, C0i = coef(x_i) / 2, Cii = coef(X_ii), Cij = coef(X_ij) / 2`` the row says
  ``<C, [[1, x^T], [x, X]]> >= 0``: valid on every PSD lifted matrix iff C is PSD, the row of a unit vector iff moreover C has
  rank one and trace 1.  Asserted: ``lambda_min(C) >= -tol ||C||_F``, every eigenvalue but the largest within ``tol ||C||_F`` of
  zero, ``|tr C - 1| <= tol`` (the trace summed in np.longdouble).
* triangle: three off-diagonal X columns of one triple and one or three x columns of it, integer coefficients +-1.  The left
  side is multilinear in x on rank-one points, so validity on the box is validity at the 8 vertices of the triple's cube, checked
  in exact integer arithmetic; a triangle inequality is moreover a facet, tight at 6 of the 8 (a valid but weaker row with a
  flipped sign is tight at 4).

Anything else -- a column outside ``[0, L + n)``, a repeated column, an incomplete pattern -- raises ``CertificateError``: the
shape test is the check on column indices.  ``eigenpair`` holds a row the round's own separation added against the LP point it
separated: ``v`` = top eigenvector of C, ``M`` = the lifted submatrix of the row's set, ``theta = v^T M v < -1e-15`` (the
library's emission threshold, held to within ``tol ||M||_F``: the emitter compared its own eigenvalue, which the eigenpair's
residual bounds the distance to) and ``||M v - theta v|| <= tol ||M||_F``.

Tolerances.  C is ``v v^T`` up to one rounding per entry (the factor 2 is exact): 2 eps ||C||_F of its own.  The rest is the error
of the host eigensolver that evaluates the certificate, measured by ``measure_tolerances`` on rows built in numpy from ``eigh``
vectors (the reference, not the code under test) and given a factor 4 per order: ``TOL`` holds the result, test_loop_cases_cpu.py
measures again, prints the figures and holds the committed ones to within a factor 2 of them; profiles/loop_pairs.txt records both.
"""
import itertools
import os
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSTANCES = os.path.join(ROOT, "tests", "golden", "instances")
BOXQP = ("spar020-100-1.in", "spar040-030-1.in")
QCQP = "q_20_4_25_1.osil"
ROUNDS = 4
SEL_SIZE = 0.1
SEED = 20

# ------------------------------------------------------------------------------------------ axes
STRATS = (0, 1, 2, 4, 5, 6, 3)                      # 3: with exact_sdp=True
FAMILIES = {"feas": (1, 5), "opt": (2, 4, 6)}       # the two routes every accepted pair of options must take
AXES = {                                            # name: (neutral value, active values)
    "tri": (False, (True,)),                        # triangle_on
    "strong": (False, (True,)),                     # strong_only
    "ch_ext": (0, (1, 2)),
    "maxpar": (None, (0.5,)),                       # max_parallel (pool_factor stays 4)
    "cuts": ((1, None), ((3, None), (5, "sets"))),  # (cuts_per_set, row_quota)
    "pool": (None, ("act",)),                       # a name of POOLS
    "box": (None, ("unit", "half")),                # a name of BOXES
    "objpar": (0.0, (0.1,)),                        # objpar_weight
}
# ages small enough to act within 4 rounds: a row slack at one optimum leaves in round 2, returns or ages from round 3 on, is
# dropped in round 4; "idle" is the neutral pool, from which nothing ever leaves
POOLS = {"act": dict(pool_max_age=1, pool_drop_age=2), "idle": dict(pool_max_age=100)}
BOXES = ("unit", "half")       # unit: (0.0, 1.0), the boxed code path on the root's box; half: 0.25 <= x_i <= 0.75 for i < n / 2

Combo = namedtuple("Combo", ("strat", "exact", "dim") + tuple(AXES))
NEUTRAL = {a: v[0] for a, v in AXES.items()}


def C(strat, dim=3, exact=None, **on):
    """the combination with strategy ``strat`` and the named axes at the given values, all others neutral"""
    for a, v in on.items():
        assert a in AXES and (v == AXES[a][0] or v in AXES[a][1] or (a == "pool" and v in POOLS)), (a, v)
    return Combo(strat=strat, exact=(strat == 3) if exact is None else bool(exact), dim=dim, **dict(NEUTRAL, **on))


def active(combo):
    """the (axis, value) pairs of a combination that are not neutral, in the order of AXES"""
    return tuple((a, getattr(combo, a)) for a in AXES if getattr(combo, a) != AXES[a][0])


def name(combo):
    """a readable id: s4-tri-cuts5sets-pool"""
    parts = ["s%d%s" % (combo.strat, "" if combo.exact == (combo.strat == 3) else "x")]
    if combo.dim != 3:
        parts.append("d%d" % combo.dim)
    for a, v in active(combo):
        if isinstance(v, bool):
            parts.append(a)
        elif a == "cuts":
            parts.append("cuts%d%s" % (v[0], v[1] or ""))
        else:
            parts.append("%s%s" % (a, v))
    return "-".join(parts)


# ------------------------------------------------------------------------------------------ the model
def accepted(combo):
    """True where ``cut_select_algo`` documents that it runs the combination, False where it documents a refusal"""
    s = combo.strat
    if s in (3, -1):
        if not combo.exact:                          # strategies 3 and -1 are the opt-in's
            return False
    elif s not in (0, 1, 2, 4, 5, 6):
        return False
    if s == 6 and combo.exact:                       # the opt-in keeps its strategy set
        return False
    if combo.objpar != 0.0 and s != 6:
        return False
    if combo.maxpar is not None and s not in (1, 2, 4, 6):
        return False
    if combo.cuts[0] > 1 and (combo.maxpar is not None or s in (0, -1)):
        return False
    if combo.pool is not None and s == 0:
        return False
    if combo.ch_ext == 2 and combo.dim != 3:
        return False
    return True


def full_product(strats=(0, 1, 2, 3, 4, 5, 6, -1), dims=(3, 4)):
    """every combination of every value of every axis, the strategies with and without the opt-in, at both dimensions"""
    values = [(AXES[a][0],) + AXES[a][1] for a in AXES]
    for s, ex, d in itertools.product(strats, (False, True), dims):
        for vals in itertools.product(*values):
            yield Combo(s, ex, d, *vals)


def box_arrays(which, n):
    if which == "unit":
        return 0.0, 1.0
    lb, ub = np.zeros(n), np.ones(n)
    lb[:n // 2], ub[:n // 2] = 0.25, 0.75
    return lb, ub


def call_kwargs(combo, n):
    """the keyword arguments of ``cut_select_algo`` for a combination on an instance of n variables; neutral values that are
    the argument's default are left out, so that a neutral axis is the call without the argument"""
    kw = dict(strat=combo.strat)
    if combo.tri:
        kw["triangle_on"] = True
    if combo.strong:
        kw["strong_only"] = True
    if combo.ch_ext:
        kw["ch_ext"] = combo.ch_ext
    if combo.maxpar is not None:
        kw["max_parallel"] = combo.maxpar
    if combo.cuts != (1, None):
        kw["cuts_per_set"], kw["row_quota"] = combo.cuts
    if combo.pool is not None:
        kw.update(POOLS[combo.pool])
    if combo.box is not None:
        kw["box"] = box_arrays(combo.box, n)
    if combo.objpar != 0.0:
        kw["objpar_weight"] = combo.objpar
    return kw


# explicit neutral values (the "B" of the neutral-value tests): the argument is passed, and must change nothing
EXPLICIT_NEUTRAL = {
    "box": lambda n: dict(box=(0.0, 1.0)),
    "cuts": lambda n: dict(cuts_per_set=1),
    "objpar": lambda n: dict(objpar_weight=0.0),
    "pool": lambda n: dict(POOLS["idle"]),
}


# ------------------------------------------------------------------------------------------ the committed combinations
# every strategy alone, then every accepted (strategy, one active option value): this contains every axis alone
ALONE = [
    C(0), C(1), C(2), C(4), C(5), C(6), C(3),
    C(0, tri=True), C(0, strong=True), C(0, ch_ext=1), C(0, ch_ext=2), C(0, box="unit"), C(0, box="half"),
    C(1, tri=True), C(1, strong=True), C(1, ch_ext=1), C(1, ch_ext=2), C(1, maxpar=0.5), C(1, cuts=(3, None)), C(1, cuts=(5, "sets")),
    C(1, pool="act"), C(1, box="unit"), C(1, box="half"),
    C(2, tri=True), C(2, strong=True), C(2, ch_ext=1), C(2, ch_ext=2), C(2, maxpar=0.5), C(2, cuts=(3, None)), C(2, cuts=(5, "sets")),
    C(2, pool="act"), C(2, box="unit"), C(2, box="half"),
    C(4, tri=True), C(4, strong=True), C(4, ch_ext=1), C(4, ch_ext=2), C(4, maxpar=0.5), C(4, cuts=(3, None)), C(4, cuts=(5, "sets")),
    C(4, pool="act"), C(4, box="unit"), C(4, box="half"),
    C(5, tri=True), C(5, strong=True), C(5, ch_ext=1), C(5, ch_ext=2), C(5, cuts=(3, None)), C(5, cuts=(5, "sets")),
    C(5, pool="act"), C(5, box="unit"), C(5, box="half"),
    C(6, tri=True), C(6, strong=True), C(6, ch_ext=1), C(6, ch_ext=2), C(6, maxpar=0.5), C(6, cuts=(3, None)), C(6, cuts=(5, "sets")),
    C(6, pool="act"), C(6, box="unit"), C(6, box="half"), C(6, objpar=0.1),
    C(3, tri=True), C(3, strong=True), C(3, ch_ext=1), C(3, ch_ext=2), C(3, cuts=(3, None)), C(3, cuts=(5, "sets")),
    C(3, pool="act"), C(3, box="unit"), C(3, box="half"),
]
# every accepted pair of active option values under a strategy of the family 1/5, the strategies taking turns
PAIRS_FEAS = [
    C(1, tri=True, strong=True), C(5, tri=True, ch_ext=1), C(1, tri=True, ch_ext=2), C(1, tri=True, maxpar=0.5),
    C(1, tri=True, cuts=(3, None)), C(5, tri=True, cuts=(5, "sets")), C(1, tri=True, pool="act"), C(5, tri=True, box="unit"),
    C(1, tri=True, box="half"), C(5, strong=True, ch_ext=1), C(1, strong=True, ch_ext=2), C(1, strong=True, maxpar=0.5),
    C(1, strong=True, cuts=(3, None)), C(5, strong=True, cuts=(5, "sets")), C(1, strong=True, pool="act"),
    C(5, strong=True, box="unit"), C(1, strong=True, box="half"), C(1, ch_ext=1, maxpar=0.5), C(1, ch_ext=1, cuts=(3, None)),
    C(5, ch_ext=1, cuts=(5, "sets")), C(1, ch_ext=1, pool="act"), C(5, ch_ext=1, box="unit"), C(1, ch_ext=1, box="half"),
    C(1, ch_ext=2, maxpar=0.5), C(1, ch_ext=2, cuts=(3, None)), C(5, ch_ext=2, cuts=(5, "sets")), C(1, ch_ext=2, pool="act"),
    C(5, ch_ext=2, box="unit"), C(1, ch_ext=2, box="half"), C(1, maxpar=0.5, pool="act"), C(1, maxpar=0.5, box="unit"),
    C(1, maxpar=0.5, box="half"), C(1, cuts=(3, None), pool="act"), C(5, cuts=(3, None), box="unit"),
    C(1, cuts=(3, None), box="half"), C(5, cuts=(5, "sets"), pool="act"), C(1, cuts=(5, "sets"), box="unit"),
    C(5, cuts=(5, "sets"), box="half"), C(1, pool="act", box="unit"), C(5, pool="act", box="half"),
]
# every accepted pair of active option values under a strategy of the family 2/4/6, the strategies taking turns
PAIRS_OPT = [
    C(2, tri=True, strong=True), C(4, tri=True, ch_ext=1), C(6, tri=True, ch_ext=2), C(2, tri=True, maxpar=0.5),
    C(4, tri=True, cuts=(3, None)), C(6, tri=True, cuts=(5, "sets")), C(2, tri=True, pool="act"), C(4, tri=True, box="unit"),
    C(6, tri=True, box="half"), C(6, tri=True, objpar=0.1), C(4, strong=True, ch_ext=1), C(6, strong=True, ch_ext=2),
    C(2, strong=True, maxpar=0.5), C(4, strong=True, cuts=(3, None)), C(6, strong=True, cuts=(5, "sets")),
    C(2, strong=True, pool="act"), C(4, strong=True, box="unit"), C(6, strong=True, box="half"), C(6, strong=True, objpar=0.1),
    C(4, ch_ext=1, maxpar=0.5), C(6, ch_ext=1, cuts=(3, None)), C(2, ch_ext=1, cuts=(5, "sets")), C(4, ch_ext=1, pool="act"),
    C(6, ch_ext=1, box="unit"), C(2, ch_ext=1, box="half"), C(6, ch_ext=1, objpar=0.1), C(6, ch_ext=2, maxpar=0.5),
    C(2, ch_ext=2, cuts=(3, None)), C(4, ch_ext=2, cuts=(5, "sets")), C(6, ch_ext=2, pool="act"), C(2, ch_ext=2, box="unit"),
    C(4, ch_ext=2, box="half"), C(6, ch_ext=2, objpar=0.1), C(2, maxpar=0.5, pool="act"), C(4, maxpar=0.5, box="unit"),
    C(6, maxpar=0.5, box="half"), C(6, maxpar=0.5, objpar=0.1), C(4, cuts=(3, None), pool="act"), C(6, cuts=(3, None), box="unit"),
    C(2, cuts=(3, None), box="half"), C(6, cuts=(3, None), objpar=0.1), C(6, cuts=(5, "sets"), pool="act"),
    C(2, cuts=(5, "sets"), box="unit"), C(4, cuts=(5, "sets"), box="half"), C(6, cuts=(5, "sets"), objpar=0.1),
    C(2, pool="act", box="unit"), C(4, pool="act", box="half"), C(6, pool="act", objpar=0.1), C(6, box="unit", objpar=0.1),
    C(6, box="half", objpar=0.1),
]
# eight triples drawn with random.Random(SEED) from the accepted ones
TRIPLES = [
    C(6, ch_ext=1, maxpar=0.5, objpar=0.1), C(6, strong=True, cuts=(3, None), objpar=0.1),
    C(5, tri=True, ch_ext=1, cuts=(5, "sets")), C(6, cuts=(3, None), box="half", objpar=0.1),
    C(4, strong=True, pool="act", box="unit"), C(4, strong=True, ch_ext=2, box="half"), C(0, strong=True, ch_ext=2, box="half"),
    C(6, strong=True, ch_ext=1, maxpar=0.5),
]
# per strategy, everything that may be on together (max_parallel and cuts_per_set exclude each other: one of the two)
EVERYTHING = [
    C(0, tri=True, strong=True, ch_ext=2, box="half"),
    C(1, tri=True, strong=True, ch_ext=2, cuts=(3, None), pool="act", box="half"),
    C(2, tri=True, strong=True, ch_ext=2, maxpar=0.5, pool="act", box="half"),
    C(4, tri=True, strong=True, ch_ext=1, cuts=(5, "sets"), pool="act", box="half"),
    C(5, tri=True, strong=True, ch_ext=2, cuts=(3, None), pool="act", box="half"),
    C(6, tri=True, strong=True, ch_ext=1, maxpar=0.5, pool="act", box="half", objpar=0.1),
    C(3, tri=True, strong=True, ch_ext=2, cuts=(3, None), pool="act", box="half"),
]

# the accepted combinations of ALONE that the neutral-value tests take as "A": one per active option value under strategy 2 (6
# for objpar_weight), and every strategy alone
NEUTRAL_A = [c for c in ALONE if not active(c)] + [c for c in ALONE if active(c) and c.strat == (6 if c.objpar else 2)]

# runs at dim 4: rows of 4 variables (14 columns) through the pool and the multi-cut path, one per strategy family
DIM4 = [C(1, dim=4, cuts=(3, None), pool="act"), C(4, dim=4, cuts=(5, "sets"), pool="act"), C(5, dim=4, cuts=(3, None), pool="act")]

COMMITTED = ALONE + PAIRS_FEAS + PAIRS_OPT + TRIPLES + EVERYTHING
assert len(set(COMMITTED)) == len(COMMITTED)


def option_pairs():
    """every unordered pair of active option values of two different axes"""
    items = [(a, v) for a in AXES for v in AXES[a][1]]
    return [(p, q) for p, q in itertools.combinations(items, 2) if p[0] != q[0]]


def uncovered_pairs(committed=None):
    """what the committed list leaves out although the model accepts it: (strategy, option value) pairs, and pairs of option
    values under a family (a pair counts as covered by a combination that has both values active, whatever else is on)"""
    committed = COMMITTED if committed is None else committed
    have = set()
    for c in committed:
        act = active(c)
        have.add((c.strat,))
        for p in act:
            have.add((c.strat, p))
        for p, q in itertools.combinations(act, 2):
            have.add((c.strat, p, q))
    missing = []
    for s in STRATS:
        if (s,) not in have:
            missing.append((s,))
        for a in AXES:
            for v in AXES[a][1]:
                if accepted(C(s, **{a: v})) and (s, (a, v)) not in have:
                    missing.append((s, (a, v)))
    for fam, strats in FAMILIES.items():
        for p, q in option_pairs():
            ok = [s for s in strats if accepted(C(s, **dict([p, q])))]
            if ok and not any((s, p, q) in have for s in ok):
                missing.append((fam, p, q))
    return missing


# ------------------------------------------------------------------------------------------ the certificate
EPS = float(np.finfo(np.float64).eps)
THRES_NEG_EIGVAL = -1e-15      # the library's emission threshold (cut_select_qp.py:24)
THRES_TRI_VIOL = 1e-7          # ... and that of a triangle inequality (:848)
# order of C (k + 1, or n + 1 for a dense row) -> worst figure measure_tolerances(SEED) gives on numpy-built rows; TOL is
# 2 eps (C's own rounding) + 4 times that
MEASURED = {
    3: 1.3323e-15,
    4: 1.6515e-15,
    5: 1.4867e-15,
    6: 1.5474e-15,
    21: 2.5524e-15,
    41: 2.9232e-15,
}
TOL = {order: 2.0 * EPS + 4.0 * worst for order, worst in MEASURED.items()}


class CertificateError(AssertionError):
    pass


_PAIRS = {}


def _pair_table(n):
    """packed position -> (i, j), i <= j, of the upper triangle stored row by row"""
    if n not in _PAIRS:
        _PAIRS[n] = np.triu_indices(n)
    return _PAIRS[n]


def packed(n, i, j):
    i, j = (i, j) if i <= j else (j, i)
    return n * i - i * (i - 1) // 2 + (j - i)


def lifted(point, n, s):
    """[[1, x^T], [x, X]] of the index set s at an LP point [X packed | x]"""
    L = n * (n + 1) // 2
    k = len(s)
    M = np.empty((k + 1, k + 1))
    M[0, 0] = 1.0
    for a in range(k):
        M[0, a + 1] = M[a + 1, 0] = point[L + s[a]]
        for b in range(a, k):
            M[a + 1, b + 1] = M[b + 1, a + 1] = point[packed(n, s[a], s[b])]
    return M


def _ld_sum(x):
    return np.sum(np.asarray(x, dtype=np.longdouble), dtype=np.longdouble)


def certify(cols, vals, rhs, n, sense="G", tol=None):
    """Hold one LP row to the certificate.  -> SimpleNamespace(kind="eig", s, C, lam_min, lam_2, trace_err, norm, order) with the
    figures relative to ||C||_F, or (kind="tri", triple, form).  Raises CertificateError.  tol: the tolerance table (TOL)."""
    tol = TOL if tol is None else tol
    L = n * (n + 1) // 2
    cols = np.asarray(cols)
    vals = np.asarray(vals, dtype=np.float64)
    if sense != "G":
        raise CertificateError("a round row of sense %r" % (sense,))
    if cols.shape != vals.shape or cols.ndim != 1 or cols.size == 0:
        raise CertificateError("columns and values do not match")
    if not np.issubdtype(cols.dtype, np.integer) or cols.min() < 0 or cols.max() >= L + n:
        raise CertificateError("a column outside [0, L + n): %r" % (cols.tolist(),))
    if np.unique(cols).size != cols.size:
        raise CertificateError("a repeated column: %r" % (cols.tolist(),))
    if not (np.all(np.isfinite(vals)) and np.isfinite(rhs)):
        raise CertificateError("a coefficient is not finite")
    coef = dict(zip(cols.tolist(), vals.tolist()))
    xs = sorted(c - L for c in coef if c >= L)
    pi, pj = _pair_table(n)
    Xs = sorted((int(pi[c]), int(pj[c])) for c in coef if c < L)
    if len(Xs) == 3 and all(i != j for i, j in Xs) and len(xs) in (1, 3):
        return _certify_triangle(coef, float(rhs), n, xs, Xs)
    k = len(xs)
    if not (2 <= k <= 5 or k == n):
        raise CertificateError("neither shape: x columns %r, X columns %r" % (xs, Xs))
    want = [(xs[a], xs[b]) for a in range(k) for b in range(a, k)]
    if Xs != want:
        raise CertificateError("the X columns are not the pairs of the set %r: %r" % (xs, Xs))
    Cm = np.empty((k + 1, k + 1))
    Cm[0, 0] = -float(rhs)
    for a in range(k):
        Cm[0, a + 1] = Cm[a + 1, 0] = coef[L + xs[a]] / 2.0
        Cm[a + 1, a + 1] = coef[packed(n, xs[a], xs[a])]
        for b in range(a + 1, k):
            Cm[a + 1, b + 1] = Cm[b + 1, a + 1] = coef[packed(n, xs[a], xs[b])] / 2.0
    order = k + 1
    if order not in tol:
        raise CertificateError("no tolerance for a row of order %d" % order)
    t = tol[order]
    norm = float(np.linalg.norm(Cm))
    if not norm > 0.0:
        raise CertificateError("an empty row")
    w = np.linalg.eigvalsh(Cm)
    out = SimpleNamespace(kind="eig", s=tuple(xs), C=Cm, order=order, norm=norm, lam_min=float(w[0]) / norm,
                          lam_2=float(np.max(np.abs(w[:-1]))) / norm, trace_err=abs(float(_ld_sum(np.diag(Cm)) - 1)))
    if out.lam_min < -t:
        raise CertificateError("not valid on the PSD cone: lambda_min(C) / ||C||_F = %.3e < -%.3e (set %r)" % (out.lam_min, t, xs))
    if out.lam_2 > t:
        raise CertificateError("not a rank-one row: |lambda_2(C)| / ||C||_F = %.3e > %.3e (set %r)" % (out.lam_2, t, xs))
    if out.trace_err > t:
        raise CertificateError("not the row of a unit vector: |tr C - 1| = %.3e > %.3e (set %r)" % (out.trace_err, t, xs))
    return out


def _certify_triangle(coef, rhs, n, xs, Xs):
    L = n * (n + 1) // 2
    triple = sorted(set(i for p in Xs for i in p))
    if len(triple) != 3 or Xs != [(triple[0], triple[1]), (triple[0], triple[2]), (triple[1], triple[2])]:
        raise CertificateError("the X columns %r are not the pairs of one triple" % (Xs,))
    if not set(xs) <= set(triple):
        raise CertificateError("x columns %r outside the triple %r" % (xs, triple))
    if any(v not in (1.0, -1.0) for v in coef.values()) or rhs != int(rhs):
        raise CertificateError("a triangle row with coefficients other than +-1: %r >= %r" % (coef, rhs))
    ic = {c: int(v) for c, v in coef.items()}
    tight = 0
    for bits in itertools.product((0, 1), repeat=3):
        x = dict(zip(triple, bits))
        lhs = sum(ic[packed(n, i, j)] * x[i] * x[j] for i, j in Xs) + sum(ic[L + i] * x[i] for i in xs)
        if lhs < int(rhs):
            raise CertificateError("a triangle row cut off the vertex %r of its cube: %r >= %r" % (bits, coef, rhs))
        tight += lhs == int(rhs)
    if tight != 6:
        raise CertificateError("a valid row on the triple %r that is no triangle inequality: tight at %d of 8 vertices" % (triple, tight))
    return SimpleNamespace(kind="tri", triple=tuple(triple), form=len(xs), which=3 if len(xs) == 3 else triple.index(xs[0]))


def row_violation(cols, vals, rhs, point):
    """rhs - a . point of a ">=" row, summed in np.longdouble: > 0 where the point violates the row"""
    return float(np.longdouble(rhs) - _ld_sum(np.asarray(vals, dtype=np.longdouble) * np.asarray(point, dtype=np.longdouble)[np.asarray(cols)]))


def eigenpair(cert, point, n, tol=None):
    """Hold an eigen-cut the round's separation added against the LP point it separated.  -> (theta, residual / ||M||_F)."""
    tol = TOL if tol is None else tol
    w, V = np.linalg.eigh(cert.C)
    v = V[:, -1].astype(np.longdouble)
    v = v / np.sqrt(_ld_sum(v * v))
    M = lifted(point, n, cert.s).astype(np.longdouble)
    Mv = np.array([_ld_sum(M[r] * v) for r in range(M.shape[0])], dtype=np.longdouble)
    theta = _ld_sum(v * Mv)
    norm = float(np.sqrt(_ld_sum(M * M)))
    resid = float(np.sqrt(_ld_sum((Mv - theta * v) ** 2))) / norm
    # the emitter compared ITS eigenvalue with the threshold, and an eigenvalue is known to within the eigenpair's residual
    # (|lambda - theta| <= ||M v - theta v||): theta is held to the threshold with the allowance the residual itself gets.  Rows
    # at the threshold exist -- theta = -9.95e-16 for a row emitted at lambda < -1e-15 -- since 1e-15 is about 4 eps ||M||_F
    if not theta < THRES_NEG_EIGVAL + tol[cert.order] * norm:
        raise CertificateError("the row of set %r is not violated at the point it was cut from: theta = %.3e" % (cert.s, float(theta)))
    if resid > tol[cert.order]:
        raise CertificateError("the row of set %r is no eigenpair of its set at the point: residual %.3e > %.3e" % (cert.s, resid, tol[cert.order]))
    return float(theta), resid


# ------------------------------------------------------------------------------------------ numpy-built rows (the reference)
def eig_row(n, s, v):
    """the eigen-cut of the vector v (order len(s) + 1) on the index set s as (cols, vals, rhs), in the library's column order:
    x columns first, then the pairs row by row"""
    L = n * (n + 1) // 2
    k = len(s)
    cols = [L + i for i in s] + [packed(n, s[a], s[b]) for a in range(k) for b in range(a, k)]
    vals = [2.0 * v[0] * v[a + 1] for a in range(k)] + [(v[a + 1] * v[b + 1]) * (1.0 if a == b else 2.0) for a in range(k) for b in range(a, k)]
    return np.array(cols, dtype=np.int64), np.array(vals, dtype=np.float64), float(-v[0] * v[0])


def tri_row(n, triple, form):
    """triangle inequality ``form`` (0..2: the one with x of triple[form]; 3: the one with all three) as (cols, vals, rhs)"""
    L = n * (n + 1) // 2
    a, b, d = triple
    X = [packed(n, a, b), packed(n, a, d), packed(n, b, d)]
    if form == 3:
        return np.array(X + [L + a, L + b, L + d], dtype=np.int64), np.array([1.0, 1.0, 1.0, -1.0, -1.0, -1.0]), -1.0
    sign = [[-1.0, -1.0, 1.0], [-1.0, 1.0, -1.0], [1.0, -1.0, -1.0]][form]
    return np.array(X + [L + triple[form]], dtype=np.int64), np.array(sign + [1.0]), 0.0


def reference_rows(seed, n, k, count):
    """``count`` numpy-built eigen-cuts of sets of k variables (k = n: the dense rows) at McCormick-feasible random points: the
    bottom eigenvector of the lifted submatrix by ``eigh``.  -> list of (cols, vals, rhs, s, point)"""
    from sdpcutsel_via_nn_amd.harness import random_mccormick_point
    rng = np.random.default_rng([seed, n, k])
    out = []
    while len(out) < count:
        point = random_mccormick_point(n, rng)
        s = tuple(sorted(rng.choice(n, size=k, replace=False).tolist()))
        w, V = np.linalg.eigh(lifted(point, n, s))
        if w[0] < -1e-6:
            out.append(eig_row(n, s, V[:, 0]) + (s, point))
    return out


def measure_tolerances(seed=SEED, count=200):
    """order -> the worst of |lambda_min| / ||C||_F, |lambda_2| / ||C||_F, |tr C - 1| and the eigenpair residual that the
    certificate computes on numpy-built rows: the error of the host eigensolver (and of eigh's own vectors), not of a device"""
    free = {o: float("inf") for o in (3, 4, 5, 6, 21, 41)}
    worst = {}
    for n, k, cnt in [(20, 2, count), (20, 3, count), (40, 4, count), (40, 5, count), (20, 20, 40), (40, 40, 20)]:
        m = 0.0
        for cols, vals, rhs, s, point in reference_rows(seed, n, k, cnt):
            c = certify(cols, vals, rhs, n, tol=free)
            m = max(m, abs(c.lam_min), c.lam_2, c.trace_err, eigenpair(c, point, n, tol=free)[1])
        worst[k + 1] = m
    return worst


# ------------------------------------------------------------------------------------------ running a combination
def store_parts(lp, first=0):
    st = lp.linear_constraints
    data, cols, lens = st.csr_parts(first)
    return np.array(data), np.array(cols), np.array(lens), np.array(st.rhs_from(first)), np.array(st.senses_from(first))


def _snapshot(cs, bound):
    lp = cs._my_prob
    run = getattr(cs, "_run", None)
    return SimpleNamespace(point=np.array(lp.get_values(), dtype=np.float64), bound=bound, rows=store_parts(lp),
                           strat=getattr(run, "strat", None),
                           pool_log=[dict(r) for r in (getattr(cs, "pool_log", None) or [])],
                           multi_log=[dict(r) for r in (getattr(cs, "multi_log", None) or [])],
                           diverse_log=[dict(r) for r in (getattr(cs, "diverse_log", None) or [])])


def _close(cs):
    """free the run's device handles now rather than when the collector gets to them"""
    seen = []
    for b in (getattr(cs, "_gpu_bindings", None) or {}).values():
        b.drain()
        seen.append(b.scorer)
    seen += [getattr(cs, a, None) for a in ("_gpu_tri", "_gpu_dense_sc")]
    seen.append(getattr(getattr(cs, "_agg_list", None), "scorer", None))
    for sc in seen:
        if sc is not None:
            sc.close()


def run_case(combo, instance, rounds=ROUNDS, sel_size=SEL_SIZE, extra=None):
    """Run ``cut_select_algo`` for a combination on a BoxQP instance of tests/golden/instances with an ``on_round`` hook that
    snapshots, at every call, the LP point, the bound, the whole row store and the run's logs.  extra(n): further keyword
    arguments (the explicit neutral values).  -> SimpleNamespace(combo, n, L, out, snaps, obj, bounds, sdp, tri, n_cand)."""
    from sdpcutsel_via_nn_amd import cut_solver
    path = os.path.join(INSTANCES, instance)
    with open(path) as f:
        n = int(f.readline().split()[0])
    cs = cut_solver.CutSolver(exact_sdp=True) if combo.exact else cut_solver.CutSolver()
    for a in ("pool_log", "multi_log", "diverse_log"):
        setattr(cs, a, None)
    snaps = []
    kw = call_kwargs(combo, n)
    if extra is not None:
        kw.update(extra(n))
    np.random.seed(SEED)            # strategy 5 shuffles with numpy's global generator
    try:
        out = cs.cut_select_algo(path, combo.dim, sel_size, nb_rounds_cuts=rounds, on_round=lambda r, log: snaps.append(_snapshot(cs, log.bounds[-1])), **kw)
        obj = np.array(cs._my_prob.obj)
    finally:
        _close(cs)
    return SimpleNamespace(combo=combo, instance=instance, n=n, L=n * (n + 1) // 2, out=out, snaps=snaps, obj=obj, bounds=[-b for b in out[0]],
                           sdp=list(out[4]), tri=list(out[5]), n_cand=out[6], pooled=combo.pool is not None or (extra is not None and "pool_max_age" in extra(n)))


def run_qcqp(strat, cuts_per_set, rounds=ROUNDS, sel_size=0.5, dim=3):
    """The QCQP loop has no hook: the round function of the instance is wrapped, so that the store and the point are seen before
    every separation, and once more after the last solve.  -> the namespace of :func:`run_case` (tri all 0)."""
    from sdpcutsel_via_nn_amd import cut_solver
    cs = cut_solver.CutSolverQCQP()
    cs.multi_log = None
    snaps = []
    inner = cs._round_qcqp

    def hooked(round_no, point):
        snaps.append(_snapshot(cs, cs._my_prob.get_objective_value()))
        return inner(round_no, point)
    cs._round_qcqp = hooked
    np.random.seed(SEED)
    try:
        out = cs.cut_select_algo(os.path.join(INSTANCES, QCQP), dim, sel_size=sel_size, strat=strat, nb_rounds_cuts=rounds, cuts_per_set=cuts_per_set)
        snaps.append(_snapshot(cs, cs._my_prob.get_objective_value()))
        obj = np.array(cs._my_prob.obj)
    finally:
        _close(cs)
        for cover in getattr(getattr(cs, "_run", None), "covers", ()):
            if getattr(cover, "scorer", None) is not None:
                cover.scorer.close()
    n = cs._nb_vars
    return SimpleNamespace(combo=C(strat, dim=dim, cuts=(cuts_per_set, None)), instance=QCQP, n=n, L=n * (n + 1) // 2, out=out, snaps=snaps, obj=obj,
                           bounds=list(out[0]), sdp=list(out[2]), tri=[0] * (len(out[2]) - 1), n_cand=None, pooled=False)


def _row_keys(rows, first):
    data, cols, lens, rhs, senses = rows
    ptr = np.concatenate([[0], np.cumsum(lens)])
    return [(cols[ptr[r]:ptr[r + 1]].astype(np.int64).tobytes(), data[ptr[r]:ptr[r + 1]].tobytes(), float(rhs[r]), str(senses[r])) for r in range(first, lens.shape[0])]


TRI_CUTS_PER_ROUND_MAX = 10000     # the loop adds every violated triangle inequality up to this many (cut_select_qp.py:844-845)


def lp_pattern(rows, n):
    """the sparsity pattern an LP was built on, read off its initial relaxation: [n, n] bool, True where an off-diagonal X_ij has a
    (McCormick) row"""
    cols = rows[1]
    pi, pj = _pair_table(n)
    c = np.unique(cols[cols < n * (n + 1) // 2])
    adj = np.zeros((n, n), dtype=bool)
    adj[pi[c], pj[c]] = True
    adj |= adj.T
    np.fill_diagonal(adj, False)
    return adj


def violated_triangles(adj, point, n):
    """The triangle inequalities of the triples a < b < d with at least two edges in ``adj`` (the ones the loop retains,
    cut_select_qp.py:812) at an LP point.  -> (must, may): sets of (triple, form) violated by more than 1e-7 beyond rounding, and by
    1e-7 within rounding.  form 0..2: -X - X + X + x of the form's variable >= 0; 3: X + X + X - x - x - x >= -1."""
    L = n * (n + 1) // 2
    a, b, d = (np.array(t) for t in zip(*itertools.combinations(range(n), 3)))
    keep = (adj[a, b].astype(int) + adj[a, d] + adj[b, d]) >= 2
    a, b, d = a[keep], b[keep], d[keep]
    p = np.asarray(point, dtype=np.longdouble)
    Xab, Xad, Xbd = (p[n * i - i * (i - 1) // 2 + (j - i)] for i, j in ((a, b), (a, d), (b, d)))
    xa, xb, xd = p[L + a], p[L + b], p[L + d]
    viol = [-(-Xab - Xad + Xbd + xa), -(-Xab + Xad - Xbd + xb), -(Xab - Xad - Xbd + xd), -1 - (Xab + Xad + Xbd - xa - xb - xd)]
    must, may = set(), set()
    for form, v in enumerate(viol):
        for t in np.flatnonzero(v >= THRES_TRI_VIOL - 8 * EPS):
            key = ((int(a[t]), int(b[t]), int(d[t])), form)
            may.add(key)
            if v[t] > THRES_TRI_VIOL + 8 * EPS:
                must.add(key)
    return must, may


def check_run(run):
    """Every round row after every round through the certificate, the rows a round's separation added through the eigenpair
    check, the row counts of the store against the tuple and the logs.  -> dict of the run's figures.  Raises AssertionError."""
    n, L, snaps = run.n, run.L, run.snaps
    n0 = snaps[0].rows[2].shape[0]                        # the initial relaxation: a stable prefix
    model_key = _row_keys(snaps[0].rows, 0)
    certs, ever = {}, set()
    fig = dict(rows=0, lam_min=0.0, lam_2=0.0, trace=0.0, resid=0.0, theta=-np.inf, tri_viol=np.inf, eig_checked=0, tri_checked=0, reentries=0)
    assert len(snaps) == len(run.bounds) and len(run.sdp) == len(snaps), (len(snaps), len(run.bounds), len(run.sdp))
    first_sets = None
    for r in range(1, len(snaps)):
        prev, cur = snaps[r - 1], snaps[r]
        data, cols, lens, rhs, senses = cur.rows
        ptr = np.concatenate([[0], np.cumsum(lens)])
        keys, before = _row_keys(cur.rows, 0), _row_keys(prev.rows, n0)
        assert keys[:n0] == model_key, "round %d: the rows of the initial relaxation changed" % r
        nrows = lens.shape[0]
        sdp, tri = run.sdp[r], run.tri[r - 1] if run.tri else 0
        added = sdp + tri
        if run.pooled:
            rec = cur.pool_log[r - 1]
            assert rec["lp_rows"] == prev.rows[2].shape[0], (r, rec, prev.rows[2].shape[0])
            assert rec["added"] == added, (r, rec, sdp, tri)
            assert nrows == rec["lp_rows"] - rec["leave"] + rec["enter"] + added, (r, rec, nrows)
            enter = rec["enter"]
            # what stays is what was there, in order; what re-enters was in the LP before, byte for byte
            stay = keys[n0:nrows - added - enter]
            it, still = iter(before), set(before)
            assert all(k in it for k in stay), "round %d: the rows that stay are no subsequence of the rows before" % r
            assert len(stay) == prev.rows[2].shape[0] - n0 - rec["leave"]
            for k in keys[nrows - added - enter:nrows - added]:
                assert k in ever and k not in still, "round %d: a re-entering row was never in the LP, or still is" % r
            fig["reentries"] += enter
        else:
            assert nrows == prev.rows[2].shape[0] + added, (r, nrows, prev.rows[2].shape[0], sdp, tri)
            assert keys[n0:nrows - added] == before, "round %d: rows of earlier rounds changed" % r
        kinds = []
        for i in range(n0, nrows):
            k = keys[i]
            if k not in certs:
                try:
                    certs[k] = certify(cols[ptr[i]:ptr[i + 1]], data[ptr[i]:ptr[i + 1]], rhs[i], n, sense=str(senses[i]))
                except CertificateError as e:
                    raise CertificateError("round %d, LP row %d (%s of the %d the round added): %s"
                                           % (r, i, "one" if i >= nrows - added else "not one", added, e))
                c = certs[k]
                if c.kind == "eig":
                    fig["lam_min"], fig["lam_2"], fig["trace"] = min(fig["lam_min"], c.lam_min), max(fig["lam_2"], c.lam_2), max(fig["trace"], c.trace_err)
            ever.add(k)
            fig["rows"] += 1
            kinds.append(certs[k].kind)
        new = kinds[len(kinds) - added:] if added else []
        assert new == ["eig"] * sdp + ["tri"] * tri, "round %d: the added rows are not %d eigen-cuts then %d triangle rows" % (r, sdp, tri)
        for i in range(nrows - added, nrows):
            c = certs[keys[i]]
            if c.kind == "eig":
                theta, resid = eigenpair(c, prev.point, n)
                fig["resid"], fig["theta"] = max(fig["resid"], resid), max(fig["theta"], theta)
                fig["eig_checked"] += 1
            else:
                viol = row_violation(cols[ptr[i]:ptr[i + 1]], data[ptr[i]:ptr[i + 1]], rhs[i], prev.point)
                # (the sum of at most 6 terms of size <= 1 that the device rounded its own way)
                assert viol >= THRES_TRI_VIOL - 8 * EPS, "round %d: the triangle row %r is violated by %.3e only" % (r, c.triple, viol)
                fig["tri_viol"] = min(fig["tri_viol"], viol)
                fig["tri_checked"] += 1
        if run.combo.tri:
            # completeness on the pattern the LP itself was built on (under ch_ext the EXTENDED one): every triangle inequality of
            # a retained triple that the point violates is among the rows the round added, and no row is of another triple
            got = set((certs[keys[i]].triple, certs[keys[i]].which) for i in range(nrows - tri, nrows))
            must, may = violated_triangles(lp_pattern(snaps[0].rows, n), prev.point, n)
            assert got <= may, "round %d: triangle rows of triples the pattern does not retain, or not violated: %r" % (r, sorted(got - may)[:5])
            if len(may) <= TRI_CUTS_PER_ROUND_MAX:
                assert must <= got, "round %d: %d violated triangle inequalities of the LP's pattern were not separated: %r" % (r, len(must - got), sorted(must - got)[:5])
        if r == 1:
            first_sets = sorted(set(certs[keys[i]].s for i in range(nrows - added, nrows - tri)))
    fig["first_sets"] = first_sets
    return fig


def resolve_from_scratch(run):
    """the final row store solved by a fresh, non-incremental LinearRelaxation -> |its optimum - the run's last bound| /
    max(1, |last bound|)"""
    from sdpcutsel_via_nn_amd import harness
    data, cols, lens, rhs, senses = run.snaps[-1].rows
    lp = harness.LinearRelaxation(run.obj, incremental=False)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    for sense in ("L", "G", "E"):
        sel = np.flatnonzero(senses == sense)
        if sel.size:
            take = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in sel])
            lp.linear_constraints.add_csr(np.concatenate([[0], np.cumsum(lens[sel])]), cols[take], data[take], rhs[sel], sense)
    assert lp.linear_constraints.get_num() == lens.shape[0]
    lp.solve()
    last = run.snaps[-1].bound
    return abs(lp.get_objective_value() - last) / max(1.0, abs(last))
