// Cut pool: what pool.hip (the step of one LP) and pool_points.hip (the read-only separation at many points, the eviction by
// serial) share -- the arrays of the pool, its workspace, the marks the compaction reads and the ONE device function for a row's
// distance d = sense * (act - rhs).  The rule is DESIGN.md section 5 "Cut pool".
#pragma once
#include "common.h"

#define POOL_LD SDPCUT_ROW_LD
#define POOL_MAX_CAP SDPCUT_POOL_MAX_ROWS

// marks of a step (PoolWs::mark)
enum { PM_LP = 0, PM_LEAVE = 1, PM_PARKED = 2, PM_VIOLATED = 3, PM_ENTER = 4, PM_DROP = 5 };
// device counters of a step (PoolWs::cnt); sdpcut_pool_drop counts the removed LP rows in word 0 and the removed parked rows in word 1
enum { PC_VIOLATED = 0, PC_LEAVE = 1, PC_DROP = 2, PC_WORDS = 4 };

// one set of the pool's arrays as the kernels take it (by value): views of a PoolArraysOwn
struct PoolArrays {
    int32_t *cols = nullptr;    // [POOL_LD][cap]
    double *vals = nullptr;     // [POOL_LD][cap]
    int32_t *nnz = nullptr, *sense = nullptr, *state = nullptr, *age = nullptr;   // [cap]
    double *rhs = nullptr, *norm = nullptr;                                       // [cap]
    int64_t *serial = nullptr;                                                    // [cap]
};

struct PoolArraysOwn {
    DevBuf<int32_t> cols, nnz, sense, state, age;
    DevBuf<double> vals, rhs, norm;
    DevBuf<int64_t> serial;
};

struct PoolWs {
    int64_t cap = 0, n = 0, next_serial = 0, n_lp = 0, n_parked = 0;
    int64_t ncols = 0;            // nb_lifted + nb_vars of the instance the columns were checked against
    PoolArraysOwn own[2];         // allocated once by sdpcut_pool_create ...
    PoolArrays a[2];              // ... and their views: the live set and the target of the next compaction
    int cur = 0;
    DevBuf<double> key;           // [cap] ranking key of a violated parked row, -inf otherwise
    DevBuf<int64_t> rowid;        // [cap] 0 .. n-1 (ascending row = ascending serial)
    DevBuf<double> key_out;       // [cap] keys of the ranked head
    DevBuf<int64_t> row_out;      // [cap] rows of the ranked head
    DevBuf<int32_t> mark;         // [cap] PM_*
    DevBuf<unsigned long long> flags, scan;   // [cap + 1] leave | dropped << 32 and its exclusive scan
    DevBuf<int32_t> ennz, eptr;               // [cap + 1] nnz of the entering rows in rank order and its exclusive scan
    DevBuf<unsigned long long> cnt;           // [PC_WORDS]
    DevBuf<char> scan_tmp;
    HostBuf stage{true};          // mapped staging of sdpcut_pool_add_csr, sdpcut_pool_separate_points, sdpcut_pool_drop
    HostBuf out{true};            // mapped block of sdpcut_pool_step / sdpcut_pool_separate_points
    // pool_points.hip: the points of a separation and the serials of an eviction on the device -- the pool's own, so that neither
    // call touches the handle's LP point (grown on demand, freed with the pool)
    DevBuf<double> d_pts;
    DevBuf<int64_t> d_drop;
};

// pool.hip
int pool_get_ws(sdpcut_ctx *h, PoolWs **out);      // the handle's pool, or SDPCUT_ESTATE: none / made for another instance
// flags[0 .. n] -> its scan, then the stable compaction of the rows not marked PM_DROP into the other set of arrays (enqueued; the
// caller waits and swaps the sets when scan[n] >> 32 rows went)
int pool_compact_enqueue(sdpcut_ctx *h, PoolWs *w, int64_t n);

#if defined(__HIPCC__)
// d = sense * (act - rhs) of row r at the point v (ncols entries): act summed left to right over the slots 0 .. nnz - 1, multiply
// and add separate
__device__ __forceinline__ double pool_row_distance(const PoolArrays &a, int64_t cap, int64_t r, int64_t ncols, const double *v)
{
#pragma clang fp contract(off)
    const int len = a.nnz[r];
    double act = 0.0;
    for (int s = 0; s < len; ++s) {
        const int32_t c = a.cols[(int64_t)s * cap + r];
        const double x = (c >= 0 && c < ncols) ? v[c] : 0.0;     // (checked when the row was added)
        act = act + a.vals[(int64_t)s * cap + r] * x;
    }
    return (double)a.sense[r] * (act - a.rhs[r]);
}
#endif
