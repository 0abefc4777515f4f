"""Triangle inequalities at tree nodes, the parts that need no device: the numpy twin (sdpcutsel_via_nn_amd/triangles.py) against
long double, against today's integer rows and against the geometry of a box; its checker against mutants; the route function and the
block layout (csrc/tri_route.h, csrc/tri_layout.h, each compiled alone with the host compiler); the front door's refusal."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import nodebox_cases
from tri_rows_numpy import numpy_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def case():
    """n = 10, a seeded pattern, its triples; a random LP point and a seeded box with all four kinds of bounds"""
    from sdpcutsel_via_nn_amd import triangles
    rng = np.random.default_rng(11)
    n = 10
    adj = np.triu(rng.uniform(size=(n, n)) < 0.7, 1)
    adj = adj | adj.T
    tri, dens = triangles.preprocess(adj)
    assert tri.shape[0] > 40 and set(dens.tolist()) == {2, 3}
    L = n * (n + 1) // 2
    vv = np.concatenate([rng.uniform(0, 1, L), rng.uniform(0, 1, n)])
    lb, ub = nodebox_cases.random_box(n, 4)
    return dict(n=n, L=L, tri=tri, dens=dens, vv=vv, box=(lb, ub), vin=nodebox_cases.point_in_box(n, lb, ub, 5))


def test_preprocess_is_the_librarys_rule():
    """>= 2 of the 3 edges, lexicographic; density 2 or 3"""
    from sdpcutsel_via_nn_amd import triangles
    adj = np.zeros((5, 5), dtype=bool)
    for i, j in ((0, 1), (1, 2), (0, 2), (2, 3)):
        adj[i, j] = adj[j, i] = True
    tri, dens = triangles.preprocess(adj)
    assert tri.tolist() == [[0, 1, 2], [0, 2, 3], [1, 2, 3]] and dens.tolist() == [3, 2, 2]


def test_violations_against_long_double(case):
    """float64 in the kernel's order against the same expressions in long double.  Without a box a violation is five roundings of
    partial sums of magnitude <= 4: within 10 eps.  With a box the table entries carry the roundings of box_X_entry -- four of
    magnitude <= 2, divided by d_i d_j, and the quotient's own -- so a violation is within (16 + 8 / min(d_i d_j)) eps (1 + max |table|)."""
    from sdpcutsel_via_nn_amd import triangles
    n, tri = case["n"], case["tri"]
    v64 = triangles.violations(tri, n, case["vv"])
    vld = triangles.violations(tri, n, case["vv"].astype(np.longdouble))
    assert v64.dtype == np.float64 and vld.dtype == np.longdouble
    assert np.abs(v64 - vld).max() <= 10 * EPS
    lb, ub = case["box"]
    t64 = triangles.point_tables(case["vin"], case["box"])
    tld = triangles.point_tables(case["vin"].astype(np.longdouble), (lb.astype(np.longdouble), ub.astype(np.longdouble)))
    d = ub - lb
    bound = (16 + 8 / (d.min() ** 2)) * EPS * (1 + np.abs(t64).max())
    err = np.abs(triangles.violations(tri, n, t64) - triangles.violations(tri, n, tld)).max()
    assert err <= bound, (err, bound)


def test_unit_box_is_todays_integer_rows(case):
    """no box and the unit box: the same bytes, and the rows _separate_and_add_triangle builds (int32 index arrays on the device)"""
    from sdpcutsel_via_nn_amd import triangles
    n, tri, dens = case["n"], case["tri"], case["dens"]
    for vv in (case["vv"], np.concatenate([np.full(case["L"], 0.75), np.full(n, 0.5)])):
        plain = triangles.round_csr(tri, dens, n, vv, 4 * tri.shape[0])
        unit = triangles.round_csr(tri, dens, n, vv, 4 * tri.shape[0], box=(np.zeros(n), np.ones(n)))
        assert plain["n_rows"] == plain["n_violated"] > 30 and triangles.same(plain, unit)
        indptr, ind, val, rhs = numpy_rows(tri, n, plain["entry"])
        assert plain["indptr"].dtype == plain["indices"].dtype == np.int32
        assert indptr.astype(np.int32).tobytes() == plain["indptr"].tobytes() and ind.astype(np.int32).tobytes() == plain["indices"].tobytes()
        assert val.tobytes() == plain["values"].tobytes() and rhs.tobytes() == plain["rhs"].tobytes()
        assert set(np.diff(plain["indptr"]).tolist()) <= {4, 6} and not np.any(np.signbit(plain["rhs"][plain["rhs"] == 0.0]))


def test_head_order_and_ties(case):
    """density 3 first, violation descending, equal keys in entry order; a NaN violates nothing"""
    from sdpcutsel_via_nn_amd import triangles
    n, tri, dens = case["n"], case["tri"], case["dens"]
    ties = np.concatenate([np.full(case["L"], 0.75), np.full(n, 0.5)])
    r = triangles.round_csr(tri, dens, n, ties, 10 ** 4)
    e = r["entry"]
    d3 = dens[e >> 2] == 3
    k = int(d3.sum())
    assert np.all(d3[:k]) and not np.any(d3[k:]) and np.all(np.diff(e[:k]) > 0) and np.all(np.diff(e[k:]) > 0) and np.all(r["viol"] == 0.25)
    bad = case["vv"].copy()
    bad[case["L"]:] = np.nan
    assert triangles.round_csr(tri, dens, n, bad, 100)["n_violated"] == 0


def test_boxed_rows_are_valid_on_the_box(case):
    """every boxed row at random (x, x x^T) with x in the box: slack >= -tol, tol = 64 eps x the magnitude the row is evaluated at"""
    from sdpcutsel_via_nn_amd import triangles
    n, L, tri = case["n"], case["L"], case["tri"]
    lb, ub = case["box"]
    indptr, ind, val, rhs = triangles.rows(tri, n, np.arange(4 * tri.shape[0]), box=case["box"])
    rng = np.random.default_rng(2)
    i, j = np.triu_indices(n)
    for _ in range(50):
        x = lb + (ub - lb) * rng.uniform(0, 1, n)
        vv = np.concatenate([x[i] * x[j], x])
        terms = val * vv[ind]
        lhs = np.add.reduceat(terms, indptr[:-1])
        mag = np.add.reduceat(np.abs(terms), indptr[:-1]) + np.abs(rhs) + 3 * np.abs(val[indptr[:-1]])
        assert np.all(lhs - rhs >= -64 * EPS * mag)


def test_boxed_rows_are_tight_where_the_facet_is(case):
    """at every vertex of the box (X = x x^T): the row's slack is the facet's in the box's variables -- 0 at the vertices where the
    facet is tight, 1 or 2 elsewhere"""
    from sdpcutsel_via_nn_amd import triangles
    n, tri = case["n"], case["tri"]
    lb, ub = case["box"]
    ent = np.arange(4 * tri.shape[0])
    indptr, ind, val, rhs = triangles.rows(tri, n, ent, box=case["box"])
    i, j = np.triu_indices(n)
    rng = np.random.default_rng(3)
    tight = 0
    for _ in range(40):
        xp = rng.integers(0, 2, n).astype(np.float64)
        x = lb + (ub - lb) * xp
        vv = np.concatenate([x[i] * x[j], x])
        terms = val * vv[ind]
        slack = np.add.reduceat(terms, indptr[:-1]) - rhs
        mag = np.add.reduceat(np.abs(terms), indptr[:-1]) + np.abs(rhs) + 3 * np.abs(val[indptr[:-1]])
        want = -triangles.violations(tri, n, np.concatenate([xp[i] * xp[j], xp])).ravel()      # exact: small integers
        assert np.all(np.abs(slack - want) <= 64 * EPS * mag)
        tight += int(np.count_nonzero(want == 0))
    assert tight > 100


def test_checker_accepts_the_twin_and_rejects_mutants(case):
    from sdpcutsel_via_nn_amd import triangles
    n, tri, dens = case["n"], case["tri"], case["dens"]
    for vv, box in ((case["vv"], None), (case["vv"], case["box"]), (case["vv"][::-1].copy(), case["box"])):
        good = triangles.round_csr(tri, dens, n, vv, 25, box=box)
        assert good["n_violated"] > 25
        args = (tri, dens, n, vv, 25)
        assert triangles.check_round(*args, good, box=box)

        def mutant(**changed):
            m = dict((k, np.array(v) if isinstance(v, np.ndarray) else v) for k, v in good.items())
            m.update(changed)
            return m

        swapped = triangles.rows(tri, n, good["entry"][[1, 0] + list(range(2, 25))], box=box)
        e = good["entry"].copy()
        e[[0, 1]] = e[[1, 0]]
        with pytest.raises(AssertionError, match="order|violation"):      # a swapped pair
            triangles.check_round(*args, mutant(entry=e, viol=good["viol"][[1, 0] + list(range(2, 25))], indptr=swapped[0], indices=swapped[1],
                                                values=swapped[2], rhs=swapped[3]), box=box)
        full = triangles.round_csr(tri, dens, n, vv, 26, box=box)      # a dropped violated entry: entry 10 of the head left out
        keep = [k for k in range(26) if k != 10]
        dropped = triangles.rows(tri, n, full["entry"][keep], box=box)
        with pytest.raises(AssertionError, match="complete"):
            triangles.check_round(*args, mutant(entry=full["entry"][keep], viol=full["viol"][keep], indptr=dropped[0], indices=dropped[1],
                                                values=dropped[2], rhs=dropped[3]), box=box)
        v = good["values"].copy()
        v[good["indptr"][3] + 1] *= -1.0
        with pytest.raises(AssertionError, match="slack"):                # a wrong sign
            triangles.check_round(*args, mutant(values=v), box=box)
        r = 5                                                              # a kept zero: a stored 0.0 on a fourth x column
        if good["indptr"][r + 1] - good["indptr"][r] < 6:
            at = int(good["indptr"][r + 1])
            ip = good["indptr"].copy()
            ip[r + 1:] += 1
            abc = tri[good["entry"][r] >> 2]
            have = set(good["indices"][good["indptr"][r]:at].tolist())
            col = max(c for c in (case["L"] + abc).tolist() if c not in have)
            assert col > good["indices"][at - 1]
            with pytest.raises(AssertionError, match="zero"):
                triangles.check_round(*args, mutant(indptr=ip, indices=np.insert(good["indices"], at, col).astype(np.int32),
                                                    values=np.insert(good["values"], at, 0.0)), box=box)
        with pytest.raises(AssertionError, match="n_violated"):
            triangles.check_round(*args, mutant(n_violated=good["n_violated"] - 1), box=box)


WRAPPER = r"""
#include "tri_route.h"
extern "C" {
int route_of(int64_t max_out, int64_t nb_vars, int64_t n_points, int boxed, int64_t budget) { return tri_route(max_out, nb_vars, n_points, boxed != 0, budget); }
int64_t table_bytes(int64_t nb_vars, int64_t n_points, int boxed) { return tri_points_table_bytes(nb_vars, n_points, boxed != 0); }
int64_t constant(int which) { return which == 0 ? TRI_POINTS_MAX_HEAD : which == 1 ? TRI_POINTS_BUDGET_BYTES : which == 2 ? TRI_POINTS_ENTRY_BYTES : TRI_FAST * 10 + TRI_LOOP; }
}
"""
WRAPPER_LAYOUT = r"""
#include "tri_layout.h"
extern "C" void layout_of(int64_t cap, int n_points, int64_t *out)
{
    const TriLayout y = tri_layout(cap);
    const TriBatchLayout b = tri_batch_layout(cap, n_points);
    const size_t v[9] = {y.entry, y.viol, y.rhs, y.values, y.indptr, y.indices, y.bytes, b.slice, b.bytes};
    for (int i = 0; i < 9; ++i) out[i] = (int64_t)v[i];
}
"""


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("tri_route")
    out = []
    for name, text in (("route", WRAPPER), ("layout", WRAPPER_LAYOUT)):      # each header alone
        src, so = d / (name + ".cpp"), d / (name + ".so")
        src.write_text(text)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)])
        out.append(ctypes.CDLL(str(so)))
    for f in (out[0].route_of, out[0].table_bytes, out[0].constant):
        f.restype = ctypes.c_int64
    out[0].route_of.argtypes = [ctypes.c_int64] * 3 + [ctypes.c_int, ctypes.c_int64]
    out[0].table_bytes.argtypes = [ctypes.c_int64] * 2 + [ctypes.c_int]
    out[1].layout_of.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
    return out


def test_route_table_at_the_boundaries(libs):
    lib = libs[0]
    FAST, LOOP = 1, 2
    assert lib.constant(3) == 12 and lib.constant(0) == 4096 and lib.constant(1) == 256 << 20 and lib.constant(2) == 12
    # the sort state of the longest head and the histogram fit the 64 KB a workgroup declares statically
    assert lib.constant(0) * lib.constant(2) + 1024 <= 64 << 10 < 2 * lib.constant(0) * lib.constant(2)
    budget = lib.constant(1)
    for boxed in (0, 1):
        assert lib.route_of(4096, 20, 256, boxed, budget) == FAST and lib.route_of(4097, 20, 256, boxed, budget) == LOOP
        assert lib.route_of(0, 20, 1, boxed, budget) == FAST and lib.route_of(16384, 20, 1, boxed, budget) == LOOP
    # the byte budget: P (L + n) doubles, twice with boxes
    for n, P in ((20, 5), (125, 256)):
        m = n * (n + 1) // 2 + n
        assert lib.table_bytes(n, P, 0) == 8 * P * m and lib.table_bytes(n, P, 1) == 16 * P * m
        for boxed in (0, 1):
            b = lib.table_bytes(n, P, boxed)
            assert lib.route_of(100, n, P, boxed, b) == FAST and lib.route_of(100, n, P, boxed, b - 1) == LOOP
    assert lib.route_of(100, 125, 256, 1, budget) == FAST      # the largest golden instance, the largest batch: 33 MB
    n = 400
    assert lib.table_bytes(n, 256, 0) <= budget < lib.table_bytes(n, 256, 1)
    assert lib.route_of(100, n, 256, 0, budget) == FAST and lib.route_of(100, n, 256, 1, budget) == LOOP


def test_layout_tiles_the_block(libs):
    out = (ctypes.c_int64 * 9)()
    for cap in (0, 1, 2, 255, 4096, 16384):
        libs[1].layout_of(cap, 5, out)
        entry, viol, rhs, values, indptr, indices, nbytes, sl, total = list(out)
        assert entry == 64 and viol == entry + 8 * cap and rhs == viol + 8 * cap and values == rhs + 8 * cap and indptr == values + 48 * cap
        assert indices >= indptr + 4 * (cap + 1) and indices % 8 == 0 and nbytes >= indices + 24 * cap and nbytes % 8 == 0
        assert sl % 64 == 0 and 0 <= sl - nbytes < 64 and total == 5 * sl


def test_abi_and_binding():
    from sdpcutsel_via_nn_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "sdpcut.h")).read()
    declared = set(re.findall(r"^int\s*(sdpcut_\w+)\s*\(", hdr, flags=re.M))
    for name in ("sdpcut_tri_round_csr", "sdpcut_tri_round_csr_points"):
        assert name in declared and name in _capi.SIGNATURES
    enums = " ".join(re.findall(r"enum\s*\{([^}]*)\}", hdr))
    stats = dict((k, int(v)) for k, v in re.findall(r"(SDPCUT_STAT_\w+)\s*=\s*(\d+)", enums))
    code = int(re.search(r"#define SDPCUT_STAT_TRI_POINTS_FAST (\d+)", hdr).group(1))
    assert code == _capi.STAT_TRI_POINTS_FAST == 19 and code not in stats.values()      # a new code behind the enumeration's, nothing renumbered
    fields = re.search(r"typedef struct sdpcut_tri_csr \{(.*?)\} sdpcut_tri_csr_t;", hdr, flags=re.S).group(1)
    names = re.findall(r"\*?(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", fields))
    assert names == [f[0] for f in _capi.TriCsr._fields_] and ctypes.sizeof(_capi.TriCsr) == 80


def test_front_door_refuses_triangle_box_without_its_partners():
    import sdpcutsel_via_nn_amd as pkg
    path = os.path.join(ROOT, "tests", "golden", "instances", "spar020-100-1.in")
    cs = pkg.CutSolver()
    for kw in (dict(triangle_box=True), dict(triangle_box=True, triangle_on=True), dict(triangle_box=True, box=(0.0, 0.5))):
        with pytest.raises(ValueError, match="triangle_box"):
            cs.cut_select_algo(path, 3, 0.1, strat=1, nb_rounds_cuts=1, **kw)
