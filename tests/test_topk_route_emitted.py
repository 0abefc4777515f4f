"""TK_ROUTE_EMITTED (csrc/topk_route.h, row 4e of the route table of DESIGN.md section 5): the refinement of TK_ROUTE_ONFLY a
selection takes exactly when the score launch emitted its strong members, the regime is resolved on the device (COMBAUTO), the head
fits 8192 entries and no shard record is written; the rest of the plan is row 4's.  With `emitted` unset nothing changes
(tests/test_topk_route.py pins that table).  CPU only: the header is plain C++."""
import ctypes
import itertools
import subprocess

import numpy as np

import test_topk_route as tr

WRAPPER = r"""
#include "topk_route.h"
extern "C" void route_one(const int64_t *a, int64_t *o)
{
    TkRouteIn r;
    r.n = a[0]; r.k = a[1]; r.mode = (int)a[2]; r.stage = (int)a[3]; r.shard_rec = a[4]; r.emitted = a[5]; r.fused_tail = a[6];
    r.pf_counted = a[7];
    const TkPlan p = tk_route(r);
    o[0] = p.err; o[1] = p.route; o[2] = p.pf_k; o[3] = p.grid_pass; o[4] = p.chunk; o[5] = p.sort_tie; o[6] = p.count_rank;
}
"""


def test_emitted_route(tmp_path):
    src = tmp_path / "route.cpp"
    src.write_text(WRAPPER)
    so = tmp_path / "route.so"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", tr.CSRC, "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    ptr = ctypes.POINTER(ctypes.c_int64)

    def route(*a):
        i, o = np.array(a, dtype=np.int64), np.zeros(7, dtype=np.int64)
        lib.route_one(i.ctypes.data_as(ptr), o.ctypes.data_as(ptr))
        return [int(v) for v in o]

    seen = 0
    for n, k, mode, stage, shard, fused, pf in itertools.product((12289, 32768, 10 ** 6), (64, 5000, 8192, 8193), (1, 2, 3, 4, 5), (0, 1, 3),
                                                                 (0, 1), (0, 1), (0, 1)):
        plain, emitted = route(n, k, mode, stage, shard, 0, fused, pf), route(n, k, mode, stage, shard, 1, fused, pf)
        want = plain[0] == 0 and plain[1] == 4 and mode == tr.COMBAUTO and not shard and k <= 8192
        if want:
            seen += 1
            assert emitted[1] == 8 and emitted[0] == 0, (n, k, mode, stage, shard, fused, pf)
            assert emitted[2:] == plain[2:]
        else:
            assert emitted == plain, (n, k, mode, stage, shard, fused, pf)
    assert seen == 3 * 3 * 2      # COMBAUTO at stage 3 with the fused tail: three lists, three heads, fine histogram counted or not
