"""Batched rounds with a node box per point (sdpcut_score_points_boxed / sdpcut_round_csr_points_boxed), the parts that need no
device: the C-ABI carries the two entry points, the route function (csrc/batch_route.h: batch_route_boxed, compiled alone with
the host compiler) is batch_route plus the byte budget of the per-point tables, and the numpy side -- nodebox.check_boxes and
nodebox.transform_tables_points, the twin of box_points_kernel -- agrees with its single-box forms."""
import ctypes
import fnmatch
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import nodebox_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")
NAMES = ("sdpcut_score_points_boxed", "sdpcut_round_csr_points_boxed")

FAST, LOOP = 1, 2
BUDGET = 256 << 20

WRAPPER = r"""
#include "batch_route.h"
extern "C" {
// in: N, cap, strat, exact_head, shard, nb_vars, n_points  ->  out: batch_route_boxed, batch_route, bytes of the box tables
void boxed_rows(long m, const int64_t *in, int64_t *out)
{
    for (long i = 0; i < m; ++i) {
        const int64_t *a = in + 7 * i;
        out[3 * i] = batch_route_boxed(a[0], a[1], (int)a[2], a[3] != 0, a[4] != 0, a[5], a[6]);
        out[3 * i + 1] = batch_route(a[0], a[1], (int)a[2], a[3] != 0, a[4] != 0);
        out[3 * i + 2] = batch_box_table_bytes(a[5], a[6]);
    }
}
int64_t budget(void) { return BATCH_BOX_BUDGET_BYTES; }
}
"""


@pytest.fixture(scope="module")
def route_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("boxed_route")
    src, so = d / "wrap.cpp", d / "wrap.so"
    src.write_text(WRAPPER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    i64p = ctypes.POINTER(ctypes.c_int64)
    lib.boxed_rows.argtypes = [ctypes.c_long, i64p, i64p]
    lib.budget.restype = ctypes.c_int64
    return lib


def _routes(lib, rows):
    a = np.ascontiguousarray(rows, dtype=np.int64)
    out = np.zeros((a.shape[0], 3), dtype=np.int64)
    i64p = ctypes.POINTER(ctypes.c_int64)
    lib.boxed_rows(a.shape[0], a.ctypes.data_as(i64p), out.ctypes.data_as(i64p))
    return out[:, 0], out[:, 1], out[:, 2]


# ------------------------------------------------------------------------------------------ ABI
def test_abi_carries_the_boxed_entry_points():
    from sdpcutsel_via_nn_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "sdpcut.h")).read()
    declared = set(re.findall(r"^int\s*(sdpcut_\w+)\s*\(", hdr, flags=re.M))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "exports.map")).read(), flags=re.S)
    globs = [g for g in re.split(r"[;\s]+", re.search(r"global:(.*?)local:", text, flags=re.S).group(1)) if g]
    c = ctypes
    dp = c.POINTER(c.c_double)
    for name in NAMES:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), (name, globs)
        # (handle, n_points, points, point_ld, lb, ub, box_ld, ...)
        assert _capi.SIGNATURES[name][:7] == [c.c_void_p, c.c_int32, dp, c.c_int64, dp, dp, c.c_int64]
    # behind the boxes: the argument lists of the unboxed calls
    assert _capi.SIGNATURES[NAMES[0]][7:] == _capi.SIGNATURES["sdpcut_score_points"][4:]
    assert _capi.SIGNATURES[NAMES[1]][7:] == _capi.SIGNATURES["sdpcut_round_csr_points"][4:]


def test_library_exports_the_boxed_entry_points():
    from sdpcutsel_via_nn_amd import build
    so = build.build(verbose=False)
    exported = set(ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", so], text=True).splitlines() if ln.strip())
    for name in NAMES:
        assert name in exported, name


# ------------------------------------------------------------------------------------------ route
def test_boxed_route_is_batch_route_and_the_budget(route_lib):
    assert route_lib.budget() == BUDGET
    ns = [1, 512, 1051, 4096, 4097, 100000]
    caps = [0, 1, 105, 512, 513]
    boxes = [(20, 1), (20, 256), (125, 256), (1000, 1), (1000, 16), (1000, 17), (1000, 256), (4000, 1), (4000, 2), (4000, 3)]
    rows = [(n, min(c, n), s, e, sh, nv, P)
            for n, c, s, e, sh, (nv, P) in itertools.product(ns, caps, (0, 1, 2, 3, 4, 5), (0, 1), (0, 1), boxes)]
    got, plain, nbytes = _routes(route_lib, rows)
    rows = np.array(rows)
    nv, P = rows[:, 5], rows[:, 6]
    assert np.array_equal(nbytes, P * (nv * (nv + 1) + nv) * 8)      # P (2 L + n) doubles
    want = np.where((plain == FAST) & (nbytes <= BUDGET), FAST, LOOP)
    assert np.array_equal(got, want)
    # every combination occurs: fast, refused by batch_route alone, refused by the budget alone
    assert (got == FAST).any() and ((plain == LOOP) & (nbytes <= BUDGET)).any() and ((plain == FAST) & (nbytes > BUDGET)).any()
    # strategies 0, 3, 5 and reference-exact heads never leave the loop
    assert np.all(got[np.isin(rows[:, 2], (0, 3, 5))] == LOOP)
    assert np.all(got[rows[:, 3] == 1] == LOOP)


@pytest.mark.parametrize("n,cap,strat,exact,shard,nv,P,want", [
    (1051, 105, 4, 0, 0, 20, 256, FAST),
    (1051, 105, 2, 0, 0, 125, 256, FAST),          # 33 MB
    (1051, 105, 2, 0, 0, 1000, 1, FAST),           # 8 MB
    (1051, 105, 2, 0, 0, 1000, 256, LOOP),         # 2 GB: the budget
    (1051, 105, 4, 0, 0, 1000, 33, FAST),          # 264.5e6 bytes <= 268 435 456
    (1051, 105, 4, 0, 0, 1000, 34, LOOP),          # 272.5e6 bytes
    (1051, 105, 1, 0, 0, 1000, 256, LOOP),         # the route does not look at the strategy's measures
    (4097, 105, 4, 0, 0, 20, 3, LOOP), (4096, 513, 4, 0, 0, 20, 3, LOOP), (1051, 0, 2, 0, 0, 20, 3, LOOP),
    (1051, 105, 0, 0, 0, 20, 3, LOOP), (1051, 105, 3, 0, 0, 20, 3, LOOP), (1051, 105, 5, 0, 0, 20, 3, LOOP),
    (1051, 105, 2, 1, 0, 20, 3, LOOP), (1051, 105, 4, 1, 0, 20, 3, LOOP),
    (1051, 105, 4, 0, 1, 20, 3, LOOP),
])
def test_boxed_route_boundaries(route_lib, n, cap, strat, exact, shard, nv, P, want):
    got, _, _ = _routes(route_lib, [(n, cap, strat, exact, shard, nv, P)])
    assert got[0] == want


# ------------------------------------------------------------------------------------------ numpy twins
@pytest.mark.parametrize("case", ["spar020", "mixed"])
def test_transform_tables_points_equals_transform_tables_per_point(case):
    from sdpcutsel_via_nn_amd import nodebox
    inst, _ = nc.instance(case)
    n = inst["nb_vars"]
    L = n * (n + 1) // 2
    Q = np.asarray(inst["Q_arr"], dtype=np.float64)
    P = 5
    boxes = np.stack([np.stack((np.zeros(n), np.ones(n)))] + [np.stack(nc.random_box(n, 300 + p)) for p in range(1, P)])
    pts = np.stack([nc.point_in_box(n, boxes[p, 0], boxes[p, 1], 300 + p, outside=(p == 2)) for p in range(P)])
    Qb, vb = nodebox.transform_tables_points(Q, pts, boxes)
    assert Qb.shape == (P, L) and vb.shape == (P, L + n) and Qb.dtype == vb.dtype == np.float64
    for p in range(P):
        tQ, tv = nodebox.transform_tables(Q, pts[p], boxes[p, 0], boxes[p, 1])
        assert np.array_equal(Qb[p].view(np.uint64), tQ.view(np.uint64)), p
        assert np.array_equal(vb[p].view(np.uint64), tv.view(np.uint64)), p
    # the unit box: the originals' bits
    assert np.array_equal(Qb[0], Q) and np.array_equal(vb[0], pts[0])
    # one point
    Q1, v1 = nodebox.transform_tables_points(Q, pts[3:4], boxes[3:4])
    assert np.array_equal(Q1[0].view(np.uint64), Qb[3].view(np.uint64)) and np.array_equal(v1[0].view(np.uint64), vb[3].view(np.uint64))


def test_check_boxes():
    from sdpcutsel_via_nn_amd import nodebox
    n, P = 20, 4
    boxes = np.stack([np.stack(nc.random_box(n, 400 + p)) for p in range(P)])
    out = nodebox.check_boxes(n, boxes)
    assert out.dtype == np.float64 and out.flags.c_contiguous and np.array_equal(out, boxes)
    assert np.array_equal(nodebox.check_boxes(n, boxes.tolist(), n_points=P), boxes)
    assert np.array_equal(nodebox.check_boxes(n, boxes[:, :, ::-1][:, :, ::-1], n_points=P), boxes)      # a view: made contiguous

    def bad(p, i, lb=None, ub=None):
        b = boxes.copy()
        if lb is not None:
            b[p, 0, i] = lb
        if ub is not None:
            b[p, 1, i] = ub
        return b

    cases = {
        "width": bad(2, 3, lb=0.25, ub=0.25 + 2.0 ** -11),
        "lb": bad(2, 3, lb=-1e-12, ub=0.5),
        "ub": bad(2, 3, lb=0.5, ub=1.0 + 1e-12),
        "nan_lb": bad(2, 3, lb=np.nan),
        "nan_ub": bad(2, 3, ub=np.nan),
        "inf_ub": bad(2, 3, ub=np.inf),
        "inf_lb": bad(2, 3, lb=-np.inf),
    }
    for tag, b in cases.items():
        with pytest.raises(ValueError, match=r"point 2\b"):
            nodebox.check_boxes(n, b)
        # the boxes in front of and behind the bad one are fine
        nodebox.check_boxes(n, b[:2])
        nodebox.check_boxes(n, b[3:])
    # the first bad point is the one named
    b = cases["width"].copy()
    b[1, 0, 0] = -0.5
    with pytest.raises(ValueError, match=r"point 1\b"):
        nodebox.check_boxes(n, b)
    # shapes
    for wrong in (boxes[:P - 1], boxes[:, :1], boxes[:, :, :n - 1], boxes[0], boxes.reshape(P, 2 * n), np.zeros((0, 2, n))):
        with pytest.raises(ValueError, match="boxes must be"):
            nodebox.check_boxes(n, wrong, n_points=P)
    nodebox.check_boxes(n, boxes[:P - 1])      # (fine without a point count)


def test_refusals_without_a_device():
    """a NULL handle (SDPCUT_EINVAL from both calls) and the Python checks of the boxes, which come before the library"""
    from sdpcutsel_via_nn_amd import _capi, build
    build.build(verbose=False)
    lib = _capi.load_library()
    pts = np.zeros((2, 9))
    bx = np.zeros((2, 2, 3))
    bx[:, 1] = 1.0
    dp = pts.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    bp = bx.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out = (_capi.RoundCsr * 2)()
    assert lib.sdpcut_score_points_boxed(None, 2, dp, 9, bp, bp, 6, _capi.EIG, dp, None) == -1
    assert lib.sdpcut_round_csr_points_boxed(None, 2, dp, 9, bp, bp, 6, 1, 1, out) == -1
    sc = _capi.Scorer.__new__(_capi.Scorer)      # no handle: the shape and box checks come first
    sc.nb_vars, sc.N = 3, 4
    narrow = bx.copy()
    narrow[1, 1, 2] = 2.0 ** -11
    for bad in (bx[:1], np.zeros((2, 2, 4)), bx[0], narrow):
        with pytest.raises(ValueError):
            sc.round_csr_points(pts, 1, 1, boxes=bad)
        with pytest.raises(ValueError):
            sc.score_points(pts, boxes=bad)
    with pytest.raises(ValueError, match=r"point 1\b"):
        sc.round_csr_points(pts, 1, 1, boxes=narrow)
    sc._h = None
