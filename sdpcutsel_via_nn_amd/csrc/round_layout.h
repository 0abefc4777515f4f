// Byte layouts of the blocks a round returns (include/sdpcut.h documents them for the caller).  Plain C++:
// tests/test_round_layout.py compiles this header with the host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

// Padded rows behind a header of hdr_bytes:  idx | score | lam | rhs | coef[entries][ld] | ks [| int32 pos[entries]]
// (sdpcut_select_round_view: hdr_bytes = 64; sdpcut_shard_finish_wait: world headers of 64 bytes, pos in the compacted form).
// No alignment padding anywhere; `bytes` ends behind ks, `bytes_pos` behind pos.
struct RowsLayout { size_t idx, score, lam, rhs, coef, ks, pos, bytes, bytes_pos; };
static inline RowsLayout rows_layout(size_t hdr_bytes, int64_t entries, int ld)
{
    RowsLayout y;
    const size_t c = (size_t)entries;
    size_t o = hdr_bytes;
    y.idx = o; o += c * 8;
    y.score = o; o += c * 8;
    y.lam = o; o += c * 8;
    y.rhs = o; o += c * 8;
    y.coef = o; o += c * (size_t)ld * 8;
    y.ks = o; o += c * 4;
    y.pos = y.bytes = o;
    y.bytes_pos = o + c * 4;
    return y;
}

// Layout of the CSR round block for `cap` head entries and rows of at most `ld` non-zeros (offsets in bytes,
// every array 8-byte aligned); the same arithmetic on the host (sdpcut_round_csr) and for the kernel's pointers.
struct CsrLayout { size_t idx, score, lam, rhs, values, ks, sets, row_entry, indptr, indices, bytes; };
static inline CsrLayout csr_layout(int64_t cap, int ld)
{
    CsrLayout y;
    const size_t c = (size_t)cap;
    auto al = [](size_t v) { return (v + 7) & ~(size_t)7; };
    size_t o = 128;
    y.idx = o; o += c * 8;
    y.score = o; o += c * 8;
    y.lam = o; o += c * 8;
    y.rhs = o; o += c * 8;
    y.values = o; o += c * (size_t)ld * 8;
    y.ks = o; o = al(o + c * 4);
    y.sets = o; o = al(o + c * 20);
    y.row_entry = o; o = al(o + c * 4);
    y.indptr = o; o = al(o + (c + 1) * 4);
    y.indices = o; o = al(o + c * (size_t)ld * 4);
    y.bytes = o;
    return y;
}

// Layout of the multi-cut round block (sdpcut_round_csr_multi): `cap` head entries, at most `row_cap` rows of at most `ld`
// non-zeros (offsets in bytes, every array 8-byte aligned).  Header of 128 bytes: int64 words 7 completion serial, 8 rows, 9
// non-zeros, 10 look-back gave up, 11 a row was dropped by the quota.  Per entry: idx | score | lam | ks | sets | n_neg; per row:
// rhs | row_lam | values | row_entry | row_rank | indptr (row_cap + 1) | indices.
struct CsrMultiLayout { size_t idx, score, lam, rhs, row_lam, values, ks, sets, n_neg, row_entry, row_rank, indptr, indices, bytes; };
static inline CsrMultiLayout csr_multi_layout(int64_t cap, int64_t row_cap, int ld)
{
    CsrMultiLayout y;
    const size_t c = (size_t)cap, r = (size_t)row_cap;
    auto al = [](size_t v) { return (v + 7) & ~(size_t)7; };
    size_t o = 128;
    y.idx = o; o += c * 8;
    y.score = o; o += c * 8;
    y.lam = o; o += c * 8;
    y.rhs = o; o += r * 8;
    y.row_lam = o; o += r * 8;
    y.values = o; o += r * (size_t)ld * 8;
    y.ks = o; o = al(o + c * 4);
    y.sets = o; o = al(o + c * 20);
    y.n_neg = o; o = al(o + c * 4);
    y.row_entry = o; o = al(o + r * 4);
    y.row_rank = o; o = al(o + r * 4);
    y.indptr = o; o = al(o + (r + 1) * 4);
    y.indices = o; o = al(o + r * (size_t)ld * 4);
    y.bytes = o;
    return y;
}
