// Byte layout of the block sdpcut_pool_separate_points returns (include/sdpcut.h documents it for the caller) and the limits of that
// call.  Plain C++, no HIP: the host code, the kernel that writes the block (pool_points.hip) and tests/test_pool_points_cpu.py
// (which compiles this header alone) read it here and nowhere else.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define POOL_POINTS_ROW_LD 20                 /* = SDPCUT_ROW_LD: most entries of a pool row */
#define POOL_POINTS_MAX_RETURN 4096           /* = SDPCUT_POOL_SEP_MAX_RETURN: most rows a point gets back */
#define POOL_POINTS_LIST 4096                 /* entries of the workgroup's list in LDS: (key bits uint64, row uint32) */
#define POOL_POINTS_ENTRY_BYTES 12
#define POOL_POINTS_HDR_BYTES 64              /* int64 words: 0 n_violated, 1 n_rows, 2 nnz, 3 select_passes */
#define POOL_POINTS_MAX_BLOCK_BYTES ((size_t)256 << 20)

#if defined(__HIPCC__)
#define POOL_POINTS_LAYOUT_FN __host__ __device__ static inline
#else
#define POOL_POINTS_LAYOUT_FN static inline
#endif

// A point's slice for `cap` = min(max_return, rows of the pool) rows: header | serial int64 [cap] | key [cap] | rhs [cap] |
// values [cap][20] | indptr int32 [cap + 1] | sense int32 [cap] | indices int32 [cap][20], padded to a multiple of 64 bytes: every
// point's header starts a cache line of its own.  The rows are packed: row i is values / indices [indptr[i], indptr[i + 1]).
struct PoolPointsLayout { size_t serial, key, rhs, values, indptr, sense, indices, slice; };
POOL_POINTS_LAYOUT_FN PoolPointsLayout pool_points_layout(int64_t cap)
{
    PoolPointsLayout y;
    const size_t c = (size_t)cap;
    size_t o = POOL_POINTS_HDR_BYTES;
    y.serial = o; o += c * 8;
    y.key = o; o += c * 8;
    y.rhs = o; o += c * 8;
    y.values = o; o += c * 8 * POOL_POINTS_ROW_LD;
    y.indptr = o; o += (c + 1) * 4;
    y.sense = o; o += c * 4;
    y.indices = o; o += c * 4 * POOL_POINTS_ROW_LD;
    y.slice = (o + 63) & ~(size_t)63;
    return y;
}

// the whole block: slice p at p * slice; refused above POOL_POINTS_MAX_BLOCK_BYTES
static inline size_t pool_points_block_bytes(int64_t cap, int n_points) { return pool_points_layout(cap).slice * (size_t)n_points; }
static inline int pool_points_block_fits(int64_t cap, int n_points) { return pool_points_block_bytes(cap, n_points) <= POOL_POINTS_MAX_BLOCK_BYTES; }
