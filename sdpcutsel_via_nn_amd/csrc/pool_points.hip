// The cut pool at tree nodes (include/sdpcut.h: sdpcut_pool_separate_points, sdpcut_pool_drop): the pool separated at P LP points in
// one call with one host wait, read-only, and rows removed by serial.  The rule is DESIGN.md section 5 "Cut pool"; cutpool.py is
// the numpy twin.
//   point copy             the P points from the pool's pinned staging to the pool's device block (the handle's LP point is not touched)
//   pool_points_kernel     one workgroup per point: counts, collects, selects, sorts and emits
// pool_points_kernel stores no key array.  Its steps, all inside the workgroup, barriers only:
//   collect   one walk over the rows: the examined violated rows are counted and, while they fit, appended to a list in LDS as
//             (key bits, row)
//   select    only where more than POOL_POINTS_LIST rows are violated: the K-th largest key over RECOMPUTED keys by radix select,
//             eight 8-bit digits from the top, a 256-bin histogram in LDS per digit; then the rows above the threshold in any order
//             and the threshold's ties in row order until K are held
//   sort      bitonic, (key descending, row ascending), in LDS: a total order, the appends' order does not matter
//   emit      the first K rows as CSR into the point's slice of the pool's pinned block (pool_points_layout.h), the header last
// There is no grid barrier and no wait on another workgroup: no give-up path (as tri_points.hip).  A workgroup per point leaves
// most of the chip idle at small P and streams the whole pool once per point -- and nine times more where the select runs.
//   pool_drop_mark_kernel  one lane per row: its serial looked up in the sorted list of the serials to remove; a hit gets the mark
//                          and the flag word the step's compaction reads (pool.hip: pool_compact_enqueue)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "pool_dev.h"
#include "pool_points_layout.h"
#include "tri_dev.h"      // tri_block_scan: the workgroup scan the triangle kernels use

#define POOL_POINTS_WAVES 16
#define POOL_POINTS_THREADS (POOL_POINTS_WAVES * 64)

static_assert(POOL_POINTS_ROW_LD == POOL_LD, "pool_points_layout.h: POOL_POINTS_ROW_LD is SDPCUT_ROW_LD");
static_assert(POOL_POINTS_MAX_RETURN == SDPCUT_POOL_SEP_MAX_RETURN, "pool_points_layout.h: POOL_POINTS_MAX_RETURN is SDPCUT_POOL_SEP_MAX_RETURN");
static_assert(POOL_POINTS_MAX_RETURN <= POOL_POINTS_LIST, "the rows a point gets back fit the list that is sorted");
static_assert((POOL_POINTS_LIST & (POOL_POINTS_LIST - 1)) == 0, "the bitonic sort pads to a power of two inside the list");
static_assert(sizeof(uint64_t) + sizeof(uint32_t) == POOL_POINTS_ENTRY_BYTES, "a list entry is key bits + row");
static_assert(POOL_POINTS_LIST * POOL_POINTS_ENTRY_BYTES + 2048 <= 64 * 1024, "the list, the histogram and the scan words fit 64 KB of LDS");

struct PoolPointsArgs {
    int64_t n, cap, ncols;
    PoolArrays a;
    const double *pts;       // [P][pts_stride]
    int64_t pts_stride;
    uint32_t state_mask;
    double viol_tol;
    int64_t max_return;      // <= POOL_POINTS_MAX_RETURN
    int64_t wcap;            // min(max_return, n): the rows a slice has room for
    char *block;
    int64_t slice;
};

// row r at the point v: examined and violated?  *bits = the bit pattern of its key (-d) / norm -- a double >= +0 or +inf, so the
// patterns order as the keys do
__device__ __forceinline__ bool pool_points_key(const PoolPointsArgs &A, const double *v, int64_t r, uint64_t *bits)
{
#pragma clang fp contract(off)
    const int st = A.a.state[r];
    if (st < 0 || st > 31 || !((1u << st) & A.state_mask)) return false;
    const double d = pool_row_distance(A.a, A.cap, r, A.ncols, v);
    const double nr = A.a.norm[r];
    if (!((-d) > A.viol_tol * nr)) return false;
    *bits = (uint64_t)__double_as_longlong((-d) / nr);
    return true;
}

// before(a, b): a stands in front of b in the result
__device__ __forceinline__ bool pool_before(uint64_t ka, uint32_t ra, uint64_t kb, uint32_t rb) { return ka > kb || (ka == kb && ra < rb); }

// LDS: 32 KB keys + 16 KB rows + 1 KB histogram + scan words = 50 256 bytes
__global__ __launch_bounds__(POOL_POINTS_THREADS) void pool_points_kernel(PoolPointsArgs A)
{
    __shared__ uint64_t s_key[POOL_POINTS_LIST];
    __shared__ uint32_t s_row[POOL_POINTS_LIST];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_wave[POOL_POINTS_WAVES];
    __shared__ uint32_t s_word[4];      // 0 n_violated, 1 the digit's bin, 2 still wanted from that bin, 3 rows collected above the threshold
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t p = blockIdx.x, n = A.n;
    const double *v = A.pts + p * A.pts_stride;
    char *block = A.block + p * A.slice;

    // collect: the counter is the list's fill while the list has room
    if (tid < 4) s_word[tid] = 0;
    __syncthreads();
    for (int64_t r = tid; r < n; r += POOL_POINTS_THREADS) {
        uint64_t k;
        if (pool_points_key(A, v, r, &k)) {
            const uint32_t at = atomicAdd(&s_word[0], 1u);
            if (at < POOL_POINTS_LIST) { s_key[at] = k; s_row[at] = (uint32_t)r; }
        }
    }
    __syncthreads();
    const uint32_t nviol = s_word[0];
    const uint32_t K = nviol < (uint64_t)A.max_return ? nviol : (uint32_t)A.max_return;      // (<= POOL_POINTS_MAX_RETURN, <= wcap)
    uint32_t held = nviol;      // the entries of the list that are sorted
    uint32_t passes = 0;

    if (nviol > POOL_POINTS_LIST && K > 0) {      // (uniform; K < nviol here)
        // select: thr = the K-th largest key, `need` of its ties wanted
        uint64_t prefix = 0, mask = 0;
        uint32_t need = K;
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            for (int64_t r = tid; r < n; r += POOL_POINTS_THREADS) {
                uint64_t k;
                if (pool_points_key(A, v, r, &k) && (k & mask) == prefix) atomicAdd(&s_hist[(k >> shift) & 255], 1u);
            }
            __syncthreads();
            if (tid < 64) {      // wave 0: lane l owns the bins 255 - 4 l .. 252 - 4 l; the bin where the count from the top reaches `need`
                uint32_t c[4], sum = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { c[j] = s_hist[255 - 4 * lane - j]; sum += c[j]; }
                uint32_t incl = sum;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t u = __shfl_up(incl, off);
                    if (lane >= off) incl += u;
                }
                uint32_t above = incl - sum;
                if (above < need && need <= incl) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (above < need && need <= above + c[j]) { s_word[1] = 255 - 4 * lane - j; s_word[2] = need - above; }
                        above += c[j];
                    }
                }
            }
            __syncthreads();
            prefix |= (uint64_t)s_word[1] << shift;
            mask |= 255ull << shift;
            need = s_word[2];
            ++passes;
        }
        const uint64_t thr = prefix;
        const uint32_t n_above = K - need;
        // the rows above the threshold in any order, the threshold's ties in row order until K are held
        uint32_t tie_run = 0;
        for (int64_t base = 0; base < n; base += POOL_POINTS_THREADS) {      // (uniform trip count: the scan holds barriers)
            const int64_t r = base + tid;
            uint64_t k = 0;
            const bool viol = r < n && pool_points_key(A, v, r, &k);
            if (viol && k > thr) {
                const uint32_t at = atomicAdd(&s_word[3], 1u);
                if (at < n_above) { s_key[at] = k; s_row[at] = (uint32_t)r; }
            }
            const uint32_t tie = viol && k == thr;
            if (tie_run < need) {      // (uniform)
                uint32_t total;
                const uint32_t at = tie_run + tri_block_scan<POOL_POINTS_WAVES>(tie, s_wave, total);
                if (tie && at < need) { s_key[n_above + at] = thr; s_row[n_above + at] = (uint32_t)r; }
                tie_run += total;
            }
        }
        held = K;
    } else if (nviol > POOL_POINTS_LIST) {
        held = 0;      // (max_return = 0: the count alone)
    }

    // sort: the held entries padded to a power of two with entries that stand last
    uint32_t n2 = 2;
    while (n2 < held) n2 <<= 1;
    __syncthreads();
    for (uint32_t i = held + tid; i < n2; i += POOL_POINTS_THREADS) { s_key[i] = 0; s_row[i] = 0xffffffffu; }
    __syncthreads();
    if (held > 1 && K > 0) {
        for (uint32_t k2 = 2; k2 <= n2; k2 <<= 1)
            for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
                for (uint32_t i = tid; i < n2; i += POOL_POINTS_THREADS) {
                    const uint32_t o = i ^ j;
                    if (o > i) {
                        const uint64_t ka = s_key[i], kb = s_key[o];
                        const uint32_t ra = s_row[i], rb = s_row[o];
                        const bool swap = (i & k2) == 0 ? pool_before(kb, rb, ka, ra) : pool_before(ka, ra, kb, rb);
                        if (swap) { s_key[i] = kb; s_key[o] = ka; s_row[i] = rb; s_row[o] = ra; }
                    }
                }
                __syncthreads();
            }
    }

    // emit
    const PoolPointsLayout y = pool_points_layout(A.wcap);
    int64_t *o_serial = (int64_t *)(block + y.serial);
    double *o_key = (double *)(block + y.key), *o_rhs = (double *)(block + y.rhs), *o_values = (double *)(block + y.values);
    int32_t *o_indptr = (int32_t *)(block + y.indptr), *o_sense = (int32_t *)(block + y.sense), *o_indices = (int32_t *)(block + y.indices);
    uint32_t run = 0;
    for (uint32_t base = 0; base < K; base += POOL_POINTS_THREADS) {      // (uniform trip count)
        const uint32_t i = base + tid;
        int64_t r = 0;
        int m = 0;
        if (i < K) {
            r = (int64_t)s_row[i];
            if (r >= n) r = 0;      // (a held row is one of the n; never an address from a stray word)
            m = A.a.nnz[r];
            m = m < 0 ? 0 : (m > POOL_LD ? POOL_LD : m);
        }
        uint32_t total;
        const uint32_t at = run + tri_block_scan<POOL_POINTS_WAVES>((uint32_t)m, s_wave, total);
        if (i < K && (int64_t)i < A.wcap) {
            o_serial[i] = A.a.serial[r];
            o_key[i] = __longlong_as_double((long long)s_key[i]);
            o_rhs[i] = A.a.rhs[r];
            o_sense[i] = A.a.sense[r];
            o_indptr[i] = (int32_t)at;
            for (int s = 0; s < m; ++s) {
                o_indices[at + s] = A.a.cols[(int64_t)s * A.cap + r];
                o_values[at + s] = A.a.vals[(int64_t)s * A.cap + r];
            }
        }
        run += total;
    }
    if (tid == 0) {
        int64_t *hdr = (int64_t *)block;
        o_indptr[K] = (int32_t)run;
        hdr[0] = (int64_t)nviol; hdr[1] = (int64_t)K; hdr[2] = (int64_t)run; hdr[3] = (int64_t)passes;
    }
}

// Row r leaves iff its serial is one of the m sorted, distinct serials of `list`: the mark and the flag word of a dropped row, as
// pool_age_kernel writes them (flags[n] = 0 closes the scan); cnt[0] / cnt[1] count the leaving rows that were in the LP / parked.
__global__ __launch_bounds__(256) void pool_drop_mark_kernel(int64_t n, int64_t m, const int64_t *list, PoolArrays a, int32_t *mark,
                                                             unsigned long long *flags, unsigned long long *cnt)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int drop = 0, parked = 0;
    if (r <= n) {
        if (r < n) {
            const int64_t s = a.serial[r];
            int64_t lo = 0, hi = m;      // the first entry >= s
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (list[mid] < s) lo = mid + 1; else hi = mid;
            }
            drop = lo < m && list[lo] == s;
            parked = a.state[r] != 0;
            mark[r] = drop ? PM_DROP : (parked ? PM_PARKED : PM_LP);
        }
        flags[r] = drop ? (1ull << 32) : 0ull;
    }
    const unsigned long long ml = __ballot(drop && !parked), mp = __ballot(drop && parked);
    if ((threadIdx.x & 63) == 0) {
        if (ml) atomicAdd(&cnt[0], (unsigned long long)__popcll(ml));
        if (mp) atomicAdd(&cnt[1], (unsigned long long)__popcll(mp));
    }
}

// ------------------------------------------------------------------------------------------
extern "C" {

int sdpcut_pool_separate_points(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, uint32_t state_mask,
                                double viol_tol, int64_t max_return, sdpcut_pool_sep_t *out)
{
    if (!h) return SDPCUT_EINVAL;
    const char *what = "sdpcut_pool_separate_points";
    PoolWs *w = nullptr;
    int rc = pool_get_ws(h, &w);
    if (rc) return rc;
    SDPCUT_NO_PENDING(h);
    if ((rc = check_point_batch(h, "", n_points, points, point_ld, w->ncols))) return rc;
    if (!out) return sdpcut_fail(h, SDPCUT_EINVAL, "out is NULL");
    if (state_mask == 0 || (state_mask & ~(uint32_t)(SDPCUT_POOL_SEP_LP | SDPCUT_POOL_SEP_PARKED)))
        return sdpcut_fail(h, SDPCUT_EINVAL, std::string(what) + ": state_mask must be SDPCUT_POOL_SEP_LP, SDPCUT_POOL_SEP_PARKED or both");
    if (!(viol_tol >= 0.0) || !std::isfinite(viol_tol)) return sdpcut_fail(h, SDPCUT_EINVAL, "viol_tol must be finite and >= 0");
    if (max_return < 0 || max_return > SDPCUT_POOL_SEP_MAX_RETURN)
        return sdpcut_fail(h, SDPCUT_EINVAL, std::string(what) + ": max_return must be 0 .. SDPCUT_POOL_SEP_MAX_RETURN (" +
                                                 std::to_string(SDPCUT_POOL_SEP_MAX_RETURN) + ")");
    const int P = n_points;
    const int64_t n = w->n, m = w->ncols;
    const int64_t wcap = max_return < n ? max_return : n;
    const PoolPointsLayout y = pool_points_layout(wcap);
    if (!pool_points_block_fits(wcap, P))
        return sdpcut_fail(h, SDPCUT_EINVAL, std::string(what) + ": the result block of " + std::to_string(P) + " points x " + std::to_string(y.slice) +
                                                 " bytes (" + std::to_string(wcap) + " rows each) = " + std::to_string(pool_points_block_bytes(wcap, P)) +
                                                 " bytes exceeds the limit of " + std::to_string(POOL_POINTS_MAX_BLOCK_BYTES) + " bytes (256 MiB)");
    std::memset(out, 0, (size_t)P * sizeof(*out));
    if (n == 0) return SDPCUT_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = grow(h, w->out, y.slice * (size_t)P))) return rc;
    if ((rc = grow(h, w->stage, (size_t)P * (size_t)m * 8))) return rc;
    if ((rc = grow(h, w->d_pts, (size_t)P * (size_t)m))) return rc;
    double *st = (double *)w->stage.get();
    pack_points(st, P, points, point_ld, m);
    HIP_TRY(h, hipMemcpyAsync(w->d_pts.get(), st, (size_t)P * m * 8, hipMemcpyHostToDevice, h->stream));
    PoolPointsArgs A;
    A.n = n;
    A.cap = w->cap;
    A.ncols = m;
    A.a = w->a[w->cur];
    A.pts = w->d_pts.get();
    A.pts_stride = m;
    A.state_mask = state_mask;
    A.viol_tol = viol_tol;
    A.max_return = max_return;
    A.wcap = wcap;
    A.block = (char *)w->out.dev();
    A.slice = (int64_t)y.slice;
    hipLaunchKernelGGL(pool_points_kernel, dim3((unsigned)P), dim3(POOL_POINTS_THREADS), 0, h->stream, A);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, sdpcut_sync(h));      // the one wait of the call
    const char *blk = (const char *)w->out.get();
    for (int p = 0; p < P; ++p) {
        const char *b = blk + y.slice * (size_t)p;
        const int64_t *hdr = (const int64_t *)b;
        sdpcut_pool_sep_t &o = out[p];
        o.n_violated = hdr[0];
        o.n_rows = hdr[1];
        o.nnz = hdr[2];
        o.select_passes = (int32_t)hdr[3];
        o.serial = (const int64_t *)(b + y.serial);
        o.key = (const double *)(b + y.key);
        o.indptr = (const int32_t *)(b + y.indptr);
        o.indices = (const int32_t *)(b + y.indices);
        o.values = (const double *)(b + y.values);
        o.rhs = (const double *)(b + y.rhs);
        o.sense = (const int32_t *)(b + y.sense);
    }
    return SDPCUT_OK;
}

int sdpcut_pool_drop(sdpcut_handle h, int64_t n, const int64_t *serials, int64_t *n_dropped)
{
    if (!h) return SDPCUT_EINVAL;
    if (n_dropped) *n_dropped = 0;
    PoolWs *w = nullptr;
    int rc = pool_get_ws(h, &w);
    if (rc) return rc;
    SDPCUT_NO_PENDING(h);
    if (n < 0) return sdpcut_fail(h, SDPCUT_EINVAL, "sdpcut_pool_drop: n must be >= 0");
    if (n > 0 && !serials) return sdpcut_fail(h, SDPCUT_EINVAL, "sdpcut_pool_drop: serials is NULL");
    // sorted and de-duplicated on the host; a serial never given cannot be in the pool
    std::vector<int64_t> list;
    list.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        if (serials[i] >= 0 && serials[i] < w->next_serial) list.push_back(serials[i]);
    std::sort(list.begin(), list.end());
    list.erase(std::unique(list.begin(), list.end()), list.end());
    const int64_t m = (int64_t)list.size(), rows = w->n;
    if (m == 0 || rows == 0) return SDPCUT_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = grow(h, w->stage, (size_t)m * 8))) return rc;
    if ((rc = grow(h, w->out, 64))) return rc;
    if ((rc = grow(h, w->d_drop, (size_t)m))) return rc;
    std::memcpy(w->stage.get(), list.data(), (size_t)m * 8);
    HIP_TRY(h, hipMemcpyAsync(w->d_drop.get(), w->stage.get(), (size_t)m * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(w->cnt.get(), 0, PC_WORDS * 8, h->stream));
    hipLaunchKernelGGL(pool_drop_mark_kernel, dim3((unsigned)((rows + 1 + 255) / 256)), dim3(256), 0, h->stream, rows, m, w->d_drop.get(), w->a[w->cur],
                       w->mark.get(), w->flags.get(), w->cnt.get());
    HIP_TRY(h, hipGetLastError());
    if ((rc = pool_compact_enqueue(h, w, rows))) return rc;
    HIP_TRY(h, hipMemcpyAsync(w->out.get(), w->cnt.get(), PC_WORDS * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));      // the one wait of the call
    const unsigned long long *c = (const unsigned long long *)w->out.get();
    const int64_t gone_lp = (int64_t)c[0], gone_parked = (int64_t)c[1], gone = gone_lp + gone_parked;
    if (gone > 0) w->cur = 1 - w->cur;
    w->n = rows - gone;
    w->n_lp -= gone_lp;
    w->n_parked -= gone_parked;
    if (n_dropped) *n_dropped = gone;
    return SDPCUT_OK;
}

} // extern "C"
