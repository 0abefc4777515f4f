"""The byte layouts of a round's blocks (csrc/round_layout.h: rows_layout, csr_layout) against the layout comments of
include/sdpcut.h, restated here and not generated from the header.  CPU only: the header is plain C++."""
import ctypes
import itertools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")

ROW_LD = 20      # SDPCUT_ROW_LD, include/sdpcut.h
ENTRIES = (1, 2, 63, 64, 65, 5000, 8192, 16384)
LDS = tuple(range(5, ROW_LD + 1))
ROWS_COLS = ("idx", "score", "lam", "rhs", "coef", "ks", "pos", "bytes", "bytes_pos")
CSR_COLS = ("idx", "score", "lam", "rhs", "values", "ks", "sets", "row_entry", "indptr", "indices", "bytes")

WRAPPER = r"""
#include "round_layout.h"
extern "C" void rows_batch(long m, const int64_t *in, int64_t *out)
{
    for (long i = 0; i < m; ++i) {
        const RowsLayout y = rows_layout((size_t)in[3 * i], in[3 * i + 1], (int)in[3 * i + 2]);
        const size_t v[%d] = { y.idx, y.score, y.lam, y.rhs, y.coef, y.ks, y.pos, y.bytes, y.bytes_pos };
        for (int j = 0; j < %d; ++j) out[%d * i + j] = (int64_t)v[j];
    }
}
extern "C" void csr_batch(long m, const int64_t *in, int64_t *out)
{
    for (long i = 0; i < m; ++i) {
        const CsrLayout y = csr_layout(in[2 * i], (int)in[2 * i + 1]);
        const size_t v[%d] = { y.idx, y.score, y.lam, y.rhs, y.values, y.ks, y.sets, y.row_entry, y.indptr, y.indices, y.bytes };
        for (int j = 0; j < %d; ++j) out[%d * i + j] = (int64_t)v[j];
    }
}
""" % ((len(ROWS_COLS),) * 3 + (len(CSR_COLS),) * 3)


def _lib(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text(WRAPPER)
    so = tmp_path / "layout.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    return ctypes.CDLL(str(so))


def _call(fn, cases, ncols):
    cases = np.ascontiguousarray(cases, dtype=np.int64)
    out = np.full((cases.shape[0], ncols), -99, dtype=np.int64)
    p64 = ctypes.POINTER(ctypes.c_int64)
    fn(ctypes.c_long(cases.shape[0]), cases.ctypes.data_as(p64), out.ctypes.data_as(p64))
    return out


def test_rows_layout_is_the_documented_block(tmp_path):
    """header | int64 idx[c] | double score[c] | double lam_min[c] | double rhs[c] | double coef[c][ld] | int32 ks[c]
    [| int32 pos[c]] -- sdpcut_select_round_view (64 reserved bytes) and sdpcut_shard_finish_round_view / _own (world headers
    of 8 int64), the arithmetic _capi.py uses in select_round and _shard_views"""
    lib = _lib(tmp_path)
    hdrs = sorted(set([64] + [64 * w for w in range(1, 9)]))
    cases = np.array(list(itertools.product(hdrs, ENTRIES, LDS)), dtype=np.int64)
    got = _call(lib.rows_batch, cases, len(ROWS_COLS))
    assert cases.shape[0] == len(hdrs) * len(ENTRIES) * len(LDS)
    for (hdr, c, ld), row in zip(cases.tolist(), got.tolist()):
        o = hdr
        want = {}
        want["idx"] = o; o += 8 * c
        want["score"] = o; o += 8 * c
        want["lam"] = o; o += 8 * c
        want["rhs"] = o; o += 8 * c
        want["coef"] = o; o += 8 * c * ld
        want["ks"] = o; o += 4 * c
        want["pos"] = want["bytes"] = o
        want["bytes_pos"] = o + 4 * c
        assert dict(zip(ROWS_COLS, row)) == want, (hdr, c, ld)
        # the sizes as _capi.py spells them
        assert want["bytes"] == hdr + c * 8 * (4 + ld) + c * 4 and want["bytes_pos"] == hdr + c * 8 * (4 + ld) + c * 8


def test_csr_layout_arrays_are_aligned_ordered_and_disjoint(tmp_path):
    """sdpcut_round_csr_t: every array of the block starts 8-byte aligned, the arrays follow each other without overlap
    given their element counts (indptr has cap + 1 entries; values / indices hold cap * row_ld) and `bytes` covers the last"""
    lib = _lib(tmp_path)
    cases = np.array(list(itertools.product(ENTRIES, LDS)), dtype=np.int64)
    got = _call(lib.csr_batch, cases, len(CSR_COLS))
    for (c, ld), row in zip(cases.tolist(), got.tolist()):
        y = dict(zip(CSR_COLS, row))
        size = dict(idx=8 * c, score=8 * c, lam=8 * c, rhs=8 * c, values=8 * c * ld, ks=4 * c, sets=4 * 5 * c, row_entry=4 * c,
                    indptr=4 * (c + 1), indices=4 * c * ld)
        end = 128      # the header: counters, completion word, n_rows / nnz / look-back mark (words 0..10)
        for name in CSR_COLS[:-1]:
            assert y[name] % 8 == 0, (name, c, ld)
            assert y[name] >= end, (name, c, ld)
            end = y[name] + size[name]
        assert y["bytes"] >= end, (c, ld)
