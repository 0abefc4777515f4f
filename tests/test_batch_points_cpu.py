"""Batched rounds (sdpcut_score_points / sdpcut_round_csr_points), the parts that need no device: the C-ABI carries the two entry
points, the route function (csrc/batch_route.h, compiled alone with the host compiler) agrees with tk_route, the batch block's
slices tile it, and the argument refusals that are decided before anything touches a device."""
import ctypes
import fnmatch
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")
NAMES = ("sdpcut_score_points", "sdpcut_round_csr_points")

FAST, LOOP = 1, 2
SMALLSORT = 1                 # TkRoute, topk_route.h
FEAS, OPT, COMBAUTO = 1, 2, 5

WRAPPER = r"""
#include "batch_route.h"
#include "topk_route.h"
extern "C" {
// in: n, cap, strat, exact_head, shard  ->  out: batch_route, tk_route's route of the fresh selection (0: refused)
void route_rows(long m, const int64_t *in, int64_t *out)
{
    for (long i = 0; i < m; ++i) {
        const int64_t *a = in + 5 * i;
        out[2 * i] = batch_route(a[0], a[1], (int)a[2], a[3] != 0, a[4] != 0);
        TkRouteIn r;
        r.n = a[0]; r.k = a[1];
        r.mode = a[2] == 1 ? TK_MODE_FEAS : a[2] == 2 ? TK_MODE_OPT : TK_MODE_COMBAUTO;
        r.stage = a[2] == 4 ? 1 : 0;
        r.shard_rec = a[4] != 0;
        const TkPlan p = tk_route(r);
        out[2 * i + 1] = p.err ? 0 : p.route;
    }
}
// -> slice bytes, block bytes, bytes of one CSR round block, offset of point p
void layout_of(int64_t cap, int ld, int n_points, int p, int64_t *out)
{
    const BatchLayout y = batch_layout(cap, ld, n_points);
    out[0] = (int64_t)y.slice; out[1] = (int64_t)y.bytes; out[2] = (int64_t)csr_layout(cap, ld).bytes;
    out[3] = (int64_t)batch_point_offset(y, p);
}
int batch_max_points(void) { return SDPCUT_BATCH_MAX_POINTS; }
int limits(int which) { return which == 0 ? TK_SMALLSORT_N : TK_TILE; }
}
"""


@pytest.fixture(scope="module")
def route_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_route")
    src, so = d / "wrap.cpp", d / "wrap.so"
    src.write_text(WRAPPER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    i64p = ctypes.POINTER(ctypes.c_int64)
    lib.route_rows.argtypes = [ctypes.c_long, i64p, i64p]
    lib.layout_of.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, i64p]
    return lib


def _routes(lib, rows):
    a = np.ascontiguousarray(rows, dtype=np.int64)
    out = np.zeros((a.shape[0], 2), dtype=np.int64)
    i64p = ctypes.POINTER(ctypes.c_int64)
    lib.route_rows(a.shape[0], a.ctypes.data_as(i64p), out.ctypes.data_as(i64p))
    return out[:, 0], out[:, 1]


def test_abi_carries_the_batched_entry_points():
    from sdpcutsel_via_nn_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "sdpcut.h")).read()
    declared = set(re.findall(r"^int\s*(sdpcut_\w+)\s*\(", hdr, flags=re.M))
    for name in NAMES:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
    assert int(re.search(r"#define SDPCUT_BATCH_MAX_POINTS (\d+)", hdr).group(1)) == 256 == _capi.BATCH_MAX_POINTS
    assert int(re.search(r"SDPCUT_STAT_POINTS_REDONE\s*=\s*(\d+)", hdr).group(1)) == _capi.STAT_POINTS_REDONE
    # the version script exports them (its patterns are globs)
    text = open(os.path.join(CSRC, "exports.map")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    globs = [g for g in re.split(r"[;\s]+", re.search(r"global:(.*?)local:", text, flags=re.S).group(1)) if g]
    for name in NAMES:
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), (name, globs)
    # the argument lists: (handle, n_points, points, point_ld, ...)
    c = ctypes
    assert _capi.SIGNATURES[NAMES[0]][:4] == [c.c_void_p, c.c_int32, c.POINTER(c.c_double), c.c_int64]
    assert _capi.SIGNATURES[NAMES[1]][:4] == [c.c_void_p, c.c_int32, c.POINTER(c.c_double), c.c_int64]
    assert _capi.SIGNATURES[NAMES[1]][-1] == c.POINTER(_capi.RoundCsr)


def test_library_exports_the_batched_entry_points():
    from sdpcutsel_via_nn_amd import build
    so = build.build(verbose=False)
    exported = set(ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", so], text=True).splitlines() if ln.strip())
    for name in NAMES:
        assert name in exported, name


def test_route_is_tk_routes_smallsort(route_lib):
    assert route_lib.batch_max_points() == 256
    nmax, tile = route_lib.limits(0), route_lib.limits(1)
    assert (nmax, tile) == (4096, 512)
    ns = [1, 2, 15, 64, 511, 512, 513, 1051, 4095, 4096, 4097, 8192, 12288, 100000]
    caps = [0, 1, 7, 105, 511, 512, 513, 4096, 5000]
    rows = [(n, min(c, n), s, e, sh) for n, c, s, e, sh in itertools.product(ns, caps, (1, 2, 4), (0, 1), (0, 1))]
    got, tk = _routes(route_lib, rows)
    rows = np.array(rows)
    want = np.where((tk == SMALLSORT) & (rows[:, 3] == 0), FAST, LOOP)
    assert np.array_equal(got, want)
    # ... which is this predicate, restated from the issue (tk_route is not restated in the header: it is called)
    n, cap, exact, shard = rows[:, 0], rows[:, 1], rows[:, 3], rows[:, 4]
    plain = np.where((cap >= 1) & (cap <= tile) & (n <= nmax) & (shard == 0) & (exact == 0), FAST, LOOP)
    assert np.array_equal(got, plain)
    assert (got == FAST).any() and (got == LOOP).any()


@pytest.mark.parametrize("n,cap,strat,exact,want", [
    (4096, 409, 4, 0, FAST), (4097, 409, 4, 0, LOOP),          # the list limit
    (4096, 512, 1, 0, FAST), (4096, 513, 1, 0, LOOP),          # the head limit
    (1051, 0, 2, 0, LOOP),                                     # nothing to select: the single-point code reports the lengths
    (1051, 105, 2, 1, LOOP), (1051, 105, 4, 1, LOOP),          # reference-exact heads
    (1051, 105, 1, 0, FAST), (1051, 105, 2, 0, FAST), (1051, 105, 4, 0, FAST),
    (1, 1, 1, 0, FAST),
    (1051, 105, 0, 0, LOOP), (1051, 105, 3, 0, LOOP), (1051, 105, 5, 0, LOOP), (1051, 105, 104, 0, LOOP),   # not served: never fast
])
def test_route_boundaries(route_lib, n, cap, strat, exact, want):
    a = np.array([[n, cap, strat, exact, 0]], dtype=np.int64)
    out = np.zeros(2, dtype=np.int64)
    i64p = ctypes.POINTER(ctypes.c_int64)
    route_lib.route_rows(1, a.ctypes.data_as(i64p), out.ctypes.data_as(i64p))
    assert out[0] == want
    a[0, 4] = 1      # a shard: never fast
    route_lib.route_rows(1, a.ctypes.data_as(i64p), out.ctypes.data_as(i64p))
    assert out[0] == LOOP


@pytest.mark.parametrize("n_points", [1, 2, 256])
@pytest.mark.parametrize("cap,ld", [(0, 9), (1, 5), (7, 9), (105, 9), (512, 20), (513, 14), (5000, 20)])
def test_block_layout(route_lib, n_points, cap, ld):
    i64p = ctypes.POINTER(ctypes.c_int64)
    out = np.zeros(4, dtype=np.int64)
    spans = []
    for p in range(n_points):
        route_lib.layout_of(cap, ld, n_points, p, out.ctypes.data_as(i64p))
        slice_b, total, used, off = (int(v) for v in out)
        assert off % 64 == 0 and slice_b % 64 == 0
        assert used <= slice_b < used + 64            # one CSR round block, padded to the next multiple of 64
        spans.append((off, off + slice_b))
    spans.sort()
    assert spans[0][0] == 0 and spans[-1][1] == total
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 == b0                               # disjoint, no gap: together exactly the reported size


def test_refusals_without_a_device():
    """What is decided before anything touches a device: a NULL handle (SDPCUT_EINVAL from both calls) and the Python checks of
    the points array's shape."""
    from sdpcutsel_via_nn_amd import _capi, build
    build.build(verbose=False)
    lib = _capi.load_library()
    pts = np.zeros((2, 9))
    dp = pts.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out = (_capi.RoundCsr * 2)()
    assert lib.sdpcut_score_points(None, 2, dp, 9, _capi.EIG, dp, None) == -1
    assert lib.sdpcut_round_csr_points(None, 2, dp, 9, 1, 1, out) == -1
    sc = _capi.Scorer.__new__(_capi.Scorer)      # no handle: the shape checks come first
    sc.nb_vars, sc.N = 3, 4
    for bad in (np.zeros(9), np.zeros((2, 8)), np.zeros((0, 9)), np.zeros((257, 9)), np.zeros((2, 3, 3))):
        with pytest.raises(ValueError):
            sc.round_csr_points(bad, 1, 1)
        with pytest.raises(ValueError):
            sc.score_points(bad)
    with pytest.raises(ValueError):
        sc.score_points(np.zeros((2, 9)), eig=False, obj=False)
    sc._h = None


def test_one_driver_for_the_plain_and_the_filtered_batch():
    """csrc/points.hip holds ONE body of the one-wait batched round (round_points; DESIGN.md section 5, "The batched round's
    driver"): each step of the chain is written once, and the two functions it replaced are gone"""
    text = open(os.path.join(CSRC, "points.hip")).read()
    once = ("hipLaunchKernelGGL(tk_points_kernel,", "launch_round_csr_points(", "rank_fast_finish(", "++h->stat_points_redone", "route = BATCH_LOOP",
            "std::memcpy(slot, h->pinned.get()", '": look-back of the row assembly timed out twice"', "launch_div_points(",
            "if (hdr[10] && o.n_out > 0) again.push_back(p);", "++h->stat_fallbacks", "static int round_points(")
    for piece in once:
        assert text.count(piece) == 1, (piece, text.count(piece))
    for gone in ("round_csr_points_impl", "round_csr_points_diverse_impl", "point_through_round"):
        assert not re.search(r"\b%s\b" % gone, text), gone
    # the three entry points fill in the description and call it
    assert len(re.findall(r"return round_points\(h, R, n_points, points, point_ld, out\);", text)) == 3
    # "the box of point p" is BoxRows' own: no caller forms the row addresses
    assert not re.search(r"(lb|ub) \+ \(size_t\)p \* (bx->|bx\.)?ld", text.replace("return lb + (size_t)p * ld;", "").replace("return ub + (size_t)p * ld;", ""))
