// Triangle rounds over a batch of LP points (sdpcut_tri_round_csr_points; tri_points.hip): which way a batch goes.  Plain C++, no HIP:
// the host code and tests/test_triangles_cpu.py (which compiles this header alone) read the route here and nowhere else.
#pragma once
#include <stddef.h>
#include <stdint.h>

enum TriRoute {
    TRI_FAST = 1,   // one point copy, (boxed: one table launch,) one launch of tri_points_kernel -- a workgroup per point --, one wait
    TRI_LOOP = 2    // the single-point call (sdpcut_tri_round_csr, in the point's box) once per point inside the call
};

// The longest head tri_points_kernel holds: its sort state -- a 64-bit key and a 32-bit entry id per head entry, 12 bytes -- lies in
// the LDS of the one workgroup that serves a point, next to the 1 KB digit histogram and the scan words.  4096 entries are 48 KB:
// with the histogram inside the 64 KB a workgroup may declare statically, and three such workgroups fit the 160 KB of a CU.
#define TRI_POINTS_MAX_HEAD 4096
#define TRI_POINTS_ENTRY_BYTES 12

// the budget of the per-point device tables (the same figure as BATCH_BOX_BUDGET_BYTES of batch_route.h, which this header does
// not include: it has to compile alone)
#define TRI_POINTS_BUDGET_BYTES ((int64_t)256 << 20)

// the device tables of a batch: the points, n_points (L + n) doubles, and as much again for the transformed points where boxes come
static inline int64_t tri_points_table_bytes(int64_t nb_vars, int64_t n_points, bool boxed)
{
    const int64_t L = nb_vars * (nb_vars + 1) / 2;
    return n_points * (L + nb_vars) * 8 * (boxed ? 2 : 1);
}

// TRI_FAST exactly when the head fits the workgroup's sort state and the tables fit the budget (`budget`: TRI_POINTS_BUDGET_BYTES;
// a parameter so that a test can send a small batch the other way)
static inline int tri_route(int64_t max_out, int64_t nb_vars, int64_t n_points, bool boxed, int64_t budget)
{
    if (max_out > TRI_POINTS_MAX_HEAD) return TRI_LOOP;
    return tri_points_table_bytes(nb_vars, n_points, boxed) <= budget ? TRI_FAST : TRI_LOOP;
}
