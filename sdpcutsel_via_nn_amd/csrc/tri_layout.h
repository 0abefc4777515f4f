// Byte layout of the block a triangle round returns (sdpcut_tri_round_csr, sdpcut_tri_round_csr_points; include/sdpcut.h documents it
// for the caller).  Plain C++, no HIP: the host code, the kernels that write the block (tri.hip, tri_points.hip) and
// tests/test_triangles_cpu.py (which compiles this header alone) read it here and nowhere else.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define TRI_ROW_LD 6          /* most non-zeros of a row: X_ab, X_ac, X_bc, x_a, x_b, x_c */
#define TRI_HDR_BYTES 64      /* int64 words: 0 n_rows, 1 n_violated, 2 nnz, 3 the selection declared itself void */

// `cap` head entries: header | entry int64 | viol | rhs | values [cap][6] | indptr int32 [cap + 1] | indices int32 [cap][6]; every array
// 8-byte aligned.  The rows are packed: row r is values / indices [indptr[r], indptr[r + 1]).
// (the kernels compute their pointers with the same function: under a HIP compiler it is a host and device function)
#if defined(__HIPCC__)
#define TRI_LAYOUT_FN __host__ __device__ static inline
#else
#define TRI_LAYOUT_FN static inline
#endif
struct TriLayout { size_t entry, viol, rhs, values, indptr, indices, bytes; };
TRI_LAYOUT_FN size_t tri_align8(size_t v) { return (v + 7) & ~(size_t)7; }
TRI_LAYOUT_FN TriLayout tri_layout(int64_t cap)
{
    TriLayout y;
    const size_t c = (size_t)cap;
    size_t o = TRI_HDR_BYTES;
    y.entry = o; o += c * 8;
    y.viol = o; o += c * 8;
    y.rhs = o; o += c * 8;
    y.values = o; o += c * TRI_ROW_LD * 8;
    y.indptr = o; o = tri_align8(o + (c + 1) * 4);
    y.indices = o; o = tri_align8(o + c * TRI_ROW_LD * 4);
    y.bytes = o;
    return y;
}

// The batch block: n_points slices, slice p at offset p * slice; a slice is one block padded to a multiple of 64 bytes, so that
// every point's header starts a cache line of its own (as batch_route.h: batch_layout).
struct TriBatchLayout { size_t slice, bytes; };
static inline TriBatchLayout tri_batch_layout(int64_t cap, int n_points)
{
    TriBatchLayout y;
    y.slice = (tri_layout(cap).bytes + 63) & ~(size_t)63;
    y.bytes = y.slice * (size_t)n_points;
    return y;
}
