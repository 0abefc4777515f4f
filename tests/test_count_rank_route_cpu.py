"""TkPlan::count_rank (csrc/topk_route.h): which selections rank their compacted entries by counting in one launch
(tk_countrank_kernel) and which keep the tile sort and the rank merge.  CPU only: the header is plain C++ and is compiled alone,
as tests/test_topk_route.py does; that test pins every other field of the plan to the route table with the option at its default,
this one pins the new field and shows that the option changes nothing else."""
import ctypes
import itertools
import subprocess

import numpy as np

from test_topk_route import CSRC, FEAS, OPT, STRONG, COMBALL, COMBAUTO

IN_COLS = ("n", "k", "mode", "stage", "fused_tail", "coop_launch", "shard_rec", "prefilter", "pf_counted", "tk_coresident", "prekeys",
           "raw", "count_rank")
OUT_COLS = ("err", "route", "maxk", "sort_tie", "big_merge", "ntiles", "grid_keys", "grid_pass", "chunk", "pf_k", "fuse_ok", "count_rank")

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
        r.tk_coresident = a[9]; r.prekeys = a[10]; r.raw = a[11]; r.count_rank = a[12];
        const TkPlan p = tk_route(r);
        o[0] = p.err; o[1] = p.route; o[2] = p.maxk; o[3] = p.sort_tie; o[4] = p.big_merge; o[5] = p.ntiles;
        o[6] = p.grid_keys; o[7] = p.grid_pass; o[8] = p.chunk; o[9] = p.pf_k;
        o[10] = tk_fuse_ok(r, r.mode == TK_MODE_COMBALL || r.mode == TK_MODE_COMBAUTO);
        o[11] = p.count_rank;
    }
}
extern "C" int default_on() { return TkRouteIn().count_rank ? 1 : 0; }
extern "C" int slices() { return TK_CR_SLICES; }
""" % (len(IN_COLS), len(OUT_COLS))

N_VALUES = [1, 512, 4096, 4097, 8192, 8193, 12288, 16384, 16385, 20000, 40000, 10 ** 6]
K_VALUES = [1, 63, 64, 65, 512, 513, 5000, 8191, 8192, 8193, 9000, 16384]


def test_count_rank_plan(tmp_path):
    src = tmp_path / "route.cpp"
    src.write_text(WRAPPER)
    so = tmp_path / "route.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    assert lib.default_on() == 1
    assert lib.slices() % 4 == 0 and lib.slices() >= 4      # whole slices per 256-thread workgroup
    p64 = ctypes.POINTER(ctypes.c_int64)
    rest = np.array(list(itertools.product((FEAS, OPT, STRONG, COMBALL, COMBAUTO), (0, 1, 3), (0, 1), (0, 1), (0, 1), (1,), (0, 1),
                                           (256,), (0, 1), (0, 1))), dtype=np.int64)
    seen = set()
    for n, k in itertools.product(N_VALUES, K_VALUES):
        outs = {}
        for opt in (0, 1):
            cases = np.empty((rest.shape[0], len(IN_COLS)), dtype=np.int64)
            cases[:, 0], cases[:, 1], cases[:, 2:12], cases[:, 12] = n, k, rest, opt
            out = np.full((cases.shape[0], len(OUT_COLS)), -99, dtype=np.int64)
            lib.route_batch(ctypes.c_long(cases.shape[0]), cases.ctypes.data_as(p64), out.ctypes.data_as(p64))
            outs[opt] = out
        c = {name: cases[:, i] for i, name in enumerate(IN_COLS)}
        off, on = outs[0], outs[1]
        # the option decides nothing but the new field: refusals, routes, grids and the fusion question are the same
        assert np.array_equal(off[:, :11], on[:, :11]), (n, k)
        assert not off[:, 11].any(), (n, k)                 # option off: the two old kernels everywhere
        ok = on[:, 0] == 0
        # on: heads that fit the merge kernel's LDS (k <= 8192), scores emitted as scores, no shard record behind the head;
        # the one-launch small route (1) has no sort tail at all
        want = (k <= 8192) & (c["raw"] == 0) & (c["shard_rec"] == 0) & (on[:, 1] != 1)
        bad = np.nonzero(ok & (on[:, 11] != want))[0]
        assert bad.size == 0, (dict(zip(IN_COLS, cases[bad[0]])), int(on[bad[0], 11]))
        assert np.array_equal(on[ok, 4] == 1, np.full(int(ok.sum()), k > 8192)), (n, k)      # big_merge as before
        seen |= set((int(k <= 8192), int(s), int(r), int(v)) for s, r, v in zip(c["shard_rec"][ok], c["raw"][ok], on[ok, 11]))
    # both sides of every condition were reached by plans that are not refused
    assert (1, 0, 0, 1) in seen and (0, 0, 0, 0) in seen and (1, 1, 0, 0) in seen and (0, 0, 1, 0) in seen
