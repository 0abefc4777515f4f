"""The route a top-k selection takes (csrc/topk_route.h: tk_route, tk_fuse_ok) against a restatement of the route table of
DESIGN.md section 5, written from the table and not generated from the header.  CPU only: the header is plain C++."""
import ctypes
import itertools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")

EINVAL, ESTATE = -1, -4      # include/sdpcut.h
FEAS, OPT, STRONG, COMBALL, COMBAUTO = 1, 2, 3, 4, 5
IN_COLS = ("n", "k", "mode", "stage", "fused_tail", "coop_launch", "shard_rec", "prefilter", "pf_counted", "tk_coresident", "prekeys", "raw")
OUT_COLS = ("err", "route", "maxk", "sort_tie", "big_merge", "ntiles", "grid_keys", "grid_pass", "chunk", "pf_k", "fuse_ok")

WRAPPER = r"""
#include "topk_route.h"
extern "C" void route_batch(long m, const int64_t *in, int64_t *out)
{
    for (long i = 0; i < m; ++i) {
        const int64_t *a = in + %d * i;
        int64_t *o = out + %d * i;
        TkRouteIn r;
        r.n = a[0]; r.k = a[1]; r.mode = (int)a[2]; r.stage = (int)a[3];
        r.fused_tail = a[4]; r.coop_launch = a[5]; r.shard_rec = a[6]; r.prefilter = a[7]; r.pf_counted = a[8];
        r.tk_coresident = a[9]; r.prekeys = a[10]; r.raw = a[11];
        const TkPlan p = tk_route(r);
        o[0] = p.err; o[1] = p.route; o[2] = p.maxk; o[3] = p.sort_tie; o[4] = p.big_merge; o[5] = p.ntiles;
        o[6] = p.grid_keys; o[7] = p.grid_pass; o[8] = p.chunk; o[9] = p.pf_k;
        o[10] = tk_fuse_ok(r, r.mode == TK_MODE_COMBALL || r.mode == TK_MODE_COMBAUTO);
    }
}
""" % (len(IN_COLS), len(OUT_COLS))


def _around(*vs):
    return [v + d for v in vs for d in (-1, 0, 1)]


N_VALUES = [1] + _around(512, 2048, 3072, 4096, 8192, 12288, 16384, 32768) + [10 ** 6, 12500000]
K_FIXED = [0, 1, 64, 511, 512, 513, 2048, 5000, 8191, 8192, 8193, 16384, 16385]      # 0 and 16385: refused


def _expected(c):
    """the table: first matching row wins; returns the OUT_COLS as arrays (fields of refused cases are not compared)"""
    n, k, mode, stage = c["n"], c["k"], c["mode"], c["stage"]
    fused, coop, shard = c["fused_tail"] != 0, c["coop_launch"] != 0, c["shard_rec"] != 0
    prekeys, raw = c["prekeys"] != 0, c["raw"] != 0
    comb = (mode == COMBALL) | (mode == COMBAUTO)
    digit_done = stage == 3
    fresh = ~digit_done & ~prekeys      # precomputed keys enter at rows 5-7
    maxk = np.where(k <= 8192, 8192, 16384)
    row1 = fresh & (k <= 512) & (n <= 4096) & ~shard
    row2 = fresh & (k <= 8192) & (n <= 12288) & (4 * k <= n) & np.where(comb, (n > 2048) & (n <= 12288), (n > 3072) & (n <= 8192))
    row3 = fresh & (n <= maxk)
    route = np.select([row1, row2, row3, digit_done, fused & coop, fused], [1, 2, 3, 4, 5, 6], 7)
    big = maxk > 8192
    err = np.select([(k < 1) | (k > 16384) | (n < 1),
                     (mode == COMBAUTO) & (stage != 1) & (stage != 3),
                     route == 1,
                     digit_done & ~fused,
                     big & (mode == COMBAUTO),
                     ~big & raw],
                    [EINVAL, ESTATE, 0, ESTATE, EINVAL, EINVAL], 0)
    sort_tie = np.select([mode == COMBAUTO, mode == COMBALL], [2, 1], 0)
    cap = np.where(fused, np.minimum(c["tk_coresident"], 1024), 1024)
    grid_pass = np.minimum(np.maximum(-(-n // 4096), 1), cap)
    chunk = np.where(grid_pass < 1, 0, -(-(-(-n // np.maximum(grid_pass, 1))) // 256) * 256)      # (no workgroup: nothing to split)
    pf_k = np.where((route == 4) & (c["prefilter"] != 0) & (c["pf_counted"] != 0) & (n >= 32768), k, 0)
    # topk_fuse_ok: stage 0, no precomputed keys, whatever stage / prekeys the grid's case has
    s0_row1 = (k <= 512) & (n <= 4096) & ~shard
    s0_row2 = (k <= 8192) & (n <= 12288) & (4 * k <= n) & np.where(comb, (n > 2048) & (n <= 12288), (n > 3072) & (n <= 8192))
    fuse_ok = ~(s0_row1 | s0_row2) & fused & ~coop & (k >= 1) & (k <= 16384) & (n > maxk)
    return dict(err=err, route=route, maxk=maxk, sort_tie=sort_tie, big_merge=big.astype(np.int64), ntiles=maxk // 512,
                grid_keys=np.minimum(-(-n // 256), 1024), grid_pass=grid_pass, chunk=chunk, pf_k=pf_k,
                fuse_ok=fuse_ok.astype(np.int64))


def test_route_table(tmp_path):
    src = tmp_path / "route.cpp"
    src.write_text(WRAPPER)
    so = tmp_path / "route.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    p64 = ctypes.POINTER(ctypes.c_int64)
    rest = list(itertools.product((FEAS, OPT, STRONG, COMBALL, COMBAUTO), (0, 1, 3), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1),
                                  (0, 256, 1024, 4096), (0, 1), (0, 1)))
    rest = np.array(rest, dtype=np.int64)
    compared = 0
    routes_seen, errs_seen = set(), set()
    for n in N_VALUES:
        q = -(-n // 4)
        ks = sorted(set(K_FIXED + [q - 1, q, q + 1]))
        for k in ks:
            cases = np.empty((rest.shape[0], len(IN_COLS)), dtype=np.int64)
            cases[:, 0] = n
            cases[:, 1] = k
            cases[:, 2:] = rest
            out = np.full((cases.shape[0], len(OUT_COLS)), -99, dtype=np.int64)
            lib.route_batch(ctypes.c_long(cases.shape[0]), cases.ctypes.data_as(p64), out.ctypes.data_as(p64))
            c = {name: cases[:, i] for i, name in enumerate(IN_COLS)}
            want = _expected(c)
            got = {name: out[:, i] for i, name in enumerate(OUT_COLS)}
            for name in ("err", "fuse_ok"):      # every case
                bad = np.nonzero(got[name] != want[name])[0]
                assert bad.size == 0, (name, dict(zip(IN_COLS, cases[bad[0]])), int(got[name][bad[0]]), int(want[name][bad[0]]))
            ok = want["err"] == 0
            for name in OUT_COLS[1:-1]:          # the plan of every case that is not refused
                bad = np.nonzero(ok & (got[name] != want[name]))[0]
                assert bad.size == 0, (name, dict(zip(IN_COLS, cases[bad[0]])), int(got[name][bad[0]]), int(want[name][bad[0]]))
            compared += cases.shape[0]
            routes_seen |= set(int(r) for r in np.unique(want["route"][ok]))
            errs_seen |= set(int(e) for e in np.unique(want["err"]))
    assert compared == sum(len(set(K_FIXED + [-(-n // 4) + d for d in (-1, 0, 1)])) for n in N_VALUES) * rest.shape[0]
    assert routes_seen == {1, 2, 3, 4, 5, 6, 7} and errs_seen == {0, EINVAL, ESTATE}      # the grid reaches every row and refusal
