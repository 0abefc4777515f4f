// Cut pool on the device (include/sdpcut.h: sdpcut_pool_*): the rows a cutting-plane loop has added, aged by their slack at
// the LP point and parked when they stay slack; parked rows are separated again at every new point and return when violated.
// The rule is DESIGN.md section 5 "Cut pool"; cutpool.py is its numpy twin, operation by operation.
//   pool_append_kernel   one lane per new row: CSR -> slots, norm, serial
//   pool_eval_kernel     one lane per row: activity at the point, ageing of the LP rows, keys of the violated parked rows
//   (merge_topk_on_device, rank.hip: the violated parked rows by (key descending, serial ascending))
//   pool_enter_kernel    the first max_return of them return to the LP
//   pool_age_kernel      the other parked rows age; flags of the leaving and the dropped rows
//   pool_emit_kernel     the three serial lists, the CSR of the entering rows and the counts into the pinned block
//   pool_compact_kernel  stable compaction of the surviving rows, out of place into the second set of arrays
// Rows are stored slot-major (cols[slot * cap + row]): a wave's 64 rows read 64 consecutive words per slot.
// The arrays, the workspace and the row-distance function are pool_dev.h's: pool_points.hip (the read-only separation at many
// points, the eviction by serial) shares them and ends its eviction with this file's scan and compaction (pool_compact_enqueue).
#include <cmath>
#include <cstring>
#include <new>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "common.h"
#include "pool_dev.h"

// the step's pinned block for n rows of which at most w return
struct PoolOutLayout {
    size_t leave, dropped, enter, key, rhs, indptr, sense, indices, values, bytes;
};
static inline PoolOutLayout pool_out_layout(int64_t n, int64_t w)
{
    PoolOutLayout y;
    size_t o = 64;                                   // header: n_violated, n_leave, n_dropped, n_enter, enter nnz
    y.leave = o; o += (size_t)n * 8;
    y.dropped = o; o += (size_t)n * 8;
    y.enter = o; o += (size_t)w * 8;
    y.key = o; o += (size_t)w * 8;
    y.rhs = o; o += (size_t)w * 8;
    y.values = o; o += (size_t)w * 8 * POOL_LD;
    y.indptr = o; o += (size_t)(w + 1) * 4;
    y.sense = o; o += (size_t)w * 4;
    y.indices = o; o += (size_t)w * 4 * POOL_LD;
    y.bytes = (o + 63) & ~(size_t)63;
    return y;
}

void free_pool_ws(sdpcut_ctx *h)
{
    delete (PoolWs *)h->pool;
    h->pool = nullptr;
}

static int pool_alloc_arrays(sdpcut_ctx *h, PoolArraysOwn *o, PoolArrays *a, size_t c)
{
    HIP_TRY(h, o->cols.reset(c * POOL_LD));
    HIP_TRY(h, o->vals.reset(c * POOL_LD));
    HIP_TRY(h, o->nnz.reset(c));
    HIP_TRY(h, o->sense.reset(c));
    HIP_TRY(h, o->state.reset(c));
    HIP_TRY(h, o->age.reset(c));
    HIP_TRY(h, o->rhs.reset(c));
    HIP_TRY(h, o->norm.reset(c));
    HIP_TRY(h, o->serial.reset(c));
    a->cols = o->cols.get(); a->vals = o->vals.get(); a->nnz = o->nnz.get(); a->sense = o->sense.get(); a->state = o->state.get();
    a->age = o->age.get(); a->rhs = o->rhs.get(); a->norm = o->norm.get(); a->serial = o->serial.get();
    return 0;
}

static inline int pool_grid(int64_t n) { return (int)((n + 255) / 256); }

// ------------------------------------------------------------------------------------------
// New rows first .. first + m - 1 from the staged CSR block.  Slots beyond a row's length hold column 0 and the value 0: every
// word of a live row is defined (the compaction copies all POOL_LD slots, sdpcut_pool_get returns them).
__global__ __launch_bounds__(256) void pool_append_kernel(int64_t m, int64_t first, int64_t cap, int64_t serial0, const int32_t *indptr,
                                                          const int32_t *indices, const double *values, const double *rhs,
                                                          const int32_t *sense, PoolArrays a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int64_t r = first + i;
    if (r >= cap) return;
    const int32_t lo = indptr[i];
    int32_t len = indptr[i + 1] - lo;
    if (len > POOL_LD) len = POOL_LD;
    double ss = 0.0;
    {
#pragma clang fp contract(off)
        for (int s = 0; s < POOL_LD; ++s) {
            const bool live = s < len;
            const double v = live ? values[lo + s] : 0.0;
            a.cols[(int64_t)s * cap + r] = live ? indices[lo + s] : 0;
            a.vals[(int64_t)s * cap + r] = v;
            if (live) ss = ss + v * v;
        }
    }
    a.nnz[r] = len;
    a.rhs[r] = rhs[i];
    a.sense[r] = sense ? sense[i] : 1;
    a.norm[r] = sqrt(ss);
    a.serial[r] = serial0 + i;
    a.state[r] = 0;
    a.age[r] = 0;
}

// Activity and distance of every row at the point v (ncols entries); the LP rows age, the parked rows get their key.
__global__ __launch_bounds__(256) void pool_eval_kernel(int64_t n, int64_t cap, int64_t ncols, const double *v, double tight_tol,
                                                        double viol_tol, int32_t max_age, PoolArrays a, double *key, int64_t *rowid,
                                                        int32_t *mark, unsigned long long *cnt)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int viol = 0, leave = 0;
    if (r < n) {
        double k = -__builtin_huge_val();
        const double nr = a.norm[r];
        int m;
        {
#pragma clang fp contract(off)
            const double d = pool_row_distance(a, cap, r, ncols, v);
            if (a.state[r] == 0) {
                const int32_t g = (d > tight_tol * nr) ? a.age[r] + 1 : 0;
                leave = g >= max_age;
                a.age[r] = leave ? 0 : g;
                if (leave) a.state[r] = 1;
                m = leave ? PM_LEAVE : PM_LP;
            } else {
                viol = (-d) > viol_tol * nr;
                if (viol) k = (-d) / nr;
                m = viol ? PM_VIOLATED : PM_PARKED;
            }
        }
        key[r] = k;
        rowid[r] = r;
        mark[r] = m;
    }
    const unsigned long long mv = __ballot(viol), ml = __ballot(leave);
    if ((threadIdx.x & 63) == 0) {
        if (mv) atomicAdd(&cnt[PC_VIOLATED], (unsigned long long)__popcll(mv));
        if (ml) atomicAdd(&cnt[PC_LEAVE], (unsigned long long)__popcll(ml));
    }
}

// Entry i of the ranked head returns iff i < min(max_return, violated); ennz[0 .. wmax] = the lengths of the returning rows
// (0 behind them and at wmax: the exclusive scan's last word is the CSR's nnz).
__global__ __launch_bounds__(256) void pool_enter_kernel(int64_t wmax, int64_t n, const int64_t *row_out, const unsigned long long *cnt,
                                                         PoolArrays a, int32_t *mark, int32_t *ennz)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > wmax) return;
    const int64_t nv = (int64_t)cnt[PC_VIOLATED];
    int32_t len = 0;
    if (i < wmax && i < nv) {
        const int64_t r = row_out[i];
        if (r >= 0 && r < n) {
            a.state[r] = 0;
            a.age[r] = 0;
            mark[r] = PM_ENTER;
            len = a.nnz[r];
        }
    }
    ennz[i] = len;
}

// The parked rows that stay parked age and drop; flags[r] = leaving | dropped << 32 (flags[n] = 0 closes the scan).
__global__ __launch_bounds__(256) void pool_age_kernel(int64_t n, int32_t drop_age, PoolArrays a, int32_t *mark, unsigned long long *flags,
                                                       unsigned long long *cnt)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int drop = 0;
    if (r <= n) {
        unsigned long long f = 0ull;
        if (r < n) {
            const int m = mark[r];
            if (m == PM_PARKED || m == PM_VIOLATED) {
                const int32_t g = a.age[r] + 1;
                a.age[r] = g;
                if (g >= drop_age) { drop = 1; mark[r] = PM_DROP; }
            }
            f = (m == PM_LEAVE ? 1ull : 0ull) | (drop ? (1ull << 32) : 0ull);
        }
        flags[r] = f;
    }
    const unsigned long long md = __ballot(drop);
    if ((threadIdx.x & 63) == 0 && md) atomicAdd(&cnt[PC_DROP], (unsigned long long)__popcll(md));
}

// Lists and entering rows into the pinned block.  Lanes 0 .. n-1 serve the rows (leave / dropped lists), lanes 0 .. wmax-1 also
// serve the ranked head (serial, key, rhs, sense and the CSR span of entering row i).
__global__ __launch_bounds__(256) void pool_emit_kernel(int64_t n, int64_t wmax, int64_t cap, PoolArrays a, const int32_t *mark,
                                                        const unsigned long long *scan, const int64_t *row_out, const double *key_out,
                                                        const int32_t *eptr, const unsigned long long *cnt, char *block, PoolOutLayout y)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) {
        const int m = mark[t];
        const unsigned long long s = scan[t];
        if (m == PM_LEAVE) ((int64_t *)(block + y.leave))[(int64_t)(s & 0xffffffffull)] = a.serial[t];
        if (m == PM_DROP) ((int64_t *)(block + y.dropped))[(int64_t)(s >> 32)] = a.serial[t];
    }
    const int64_t nv = (int64_t)cnt[PC_VIOLATED];
    const int64_t w = nv < wmax ? nv : wmax;
    if (t < w) {
        const int64_t r = row_out[t];
        if (r >= 0 && r < n) {
            const int32_t lo = eptr[t];
            const int len = a.nnz[r];
            ((int64_t *)(block + y.enter))[t] = a.serial[r];
            ((double *)(block + y.key))[t] = key_out[t];
            ((double *)(block + y.rhs))[t] = a.rhs[r];
            ((int32_t *)(block + y.sense))[t] = a.sense[r];
            ((int32_t *)(block + y.indptr))[t] = lo;
            for (int s = 0; s < len; ++s) {
                ((int32_t *)(block + y.indices))[lo + s] = a.cols[(int64_t)s * cap + r];
                ((double *)(block + y.values))[lo + s] = a.vals[(int64_t)s * cap + r];
            }
        }
    }
    if (t == 0) {
        int64_t *hdr = (int64_t *)block;
        const unsigned long long tot = scan[n];
        hdr[0] = nv;
        hdr[1] = (int64_t)(tot & 0xffffffffull);
        hdr[2] = (int64_t)(tot >> 32);
        hdr[3] = w;
        hdr[4] = eptr[wmax];
        ((int32_t *)(block + y.indptr))[w] = eptr[wmax];
    }
}

// Surviving row r moves to position r - (dropped rows in front of it) of the other set of arrays.  Nothing dropped: nothing
// to do, the host keeps the live set.
__global__ __launch_bounds__(256) void pool_compact_kernel(int64_t n, int64_t cap, PoolArrays a, PoolArrays b, const int32_t *mark,
                                                           const unsigned long long *scan)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    if ((scan[n] >> 32) == 0ull) return;
    if (mark[r] == PM_DROP) return;
    const int64_t q = r - (int64_t)(scan[r] >> 32);
    if (q < 0 || q >= cap) return;
    for (int s = 0; s < POOL_LD; ++s) {
        b.cols[(int64_t)s * cap + q] = a.cols[(int64_t)s * cap + r];
        b.vals[(int64_t)s * cap + q] = a.vals[(int64_t)s * cap + r];
    }
    b.nnz[q] = a.nnz[r];
    b.sense[q] = a.sense[r];
    b.state[q] = a.state[r];
    b.age[q] = a.age[r];
    b.rhs[q] = a.rhs[r];
    b.norm[q] = a.norm[r];
    b.serial[q] = a.serial[r];
}

// ------------------------------------------------------------------------------------------
int pool_get_ws(sdpcut_ctx *h, PoolWs **out)
{
    PoolWs *w = (PoolWs *)h->pool;
    if (!w) return sdpcut_fail(h, SDPCUT_ESTATE, "sdpcut_pool_create first");
    if (w->ncols != h->L + h->nb_vars)
        return sdpcut_fail(h, SDPCUT_ESTATE, "the instance changed since sdpcut_pool_create: destroy the pool and create it again");
    *out = w;
    return 0;
}

int pool_compact_enqueue(sdpcut_ctx *h, PoolWs *w, int64_t n)
{
    size_t tb = w->scan_tmp.size();
    HIP_TRY(h, rocprim::exclusive_scan(w->scan_tmp.get(), tb, w->flags.get(), w->scan.get(), 0ull, (size_t)(n + 1), rocprim::plus<unsigned long long>(),
                                       h->stream));
    hipLaunchKernelGGL(pool_compact_kernel, dim3(pool_grid(n + 1)), dim3(256), 0, h->stream, n, w->cap, w->a[w->cur], w->a[1 - w->cur],
                       w->mark.get(), w->scan.get());
    HIP_TRY(h, hipGetLastError());
    return 0;
}

extern "C" {

int sdpcut_pool_create(sdpcut_handle h, int64_t capacity)
{
    if (!h) return SDPCUT_EINVAL;
    if (capacity < 1 || capacity > POOL_MAX_CAP) return sdpcut_fail(h, SDPCUT_EINVAL, "capacity must lie in 1 .. SDPCUT_POOL_MAX_ROWS");
    if (h->nb_vars == 0) return sdpcut_fail(h, SDPCUT_ESTATE, "set_instance first");
    SDPCUT_NO_PENDING(h);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sdpcut_sync(h));
    free_pool_ws(h);
    PoolWs *w = new (std::nothrow) PoolWs();
    if (!w) return sdpcut_fail(h, SDPCUT_ENOMEM, "out of host memory");
    h->pool = w;
    const size_t c = (size_t)capacity;
    int rc = pool_alloc_arrays(h, &w->own[0], &w->a[0], c);
    if (!rc) rc = pool_alloc_arrays(h, &w->own[1], &w->a[1], c);
    if (rc) { free_pool_ws(h); return rc; }
    hipError_t e = w->key.reset(c);
    if (e == hipSuccess) e = w->rowid.reset(c);
    if (e == hipSuccess) e = w->key_out.reset(c);
    if (e == hipSuccess) e = w->row_out.reset(c);
    if (e == hipSuccess) e = w->mark.reset(c);
    if (e == hipSuccess) e = w->flags.reset(c + 1);
    if (e == hipSuccess) e = w->scan.reset(c + 1);
    if (e == hipSuccess) e = w->ennz.reset(c + 1);
    if (e == hipSuccess) e = w->eptr.reset(c + 1);
    if (e == hipSuccess) e = w->cnt.reset(PC_WORDS);
    size_t t1 = 0, t2 = 0;
    if (e == hipSuccess)
        e = rocprim::exclusive_scan(nullptr, t1, w->flags.get(), w->scan.get(), 0ull, c + 1, rocprim::plus<unsigned long long>(), h->stream);
    if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, t2, w->ennz.get(), w->eptr.get(), 0, c + 1, rocprim::plus<int32_t>(), h->stream);
    if (e == hipSuccess) e = w->scan_tmp.reset((t1 > t2 ? t1 : t2) + 256);
    if (e != hipSuccess) {
        free_pool_ws(h);
        return sdpcut_fail(h, SDPCUT_EHIP, std::string("sdpcut_pool_create: ") + hipGetErrorString(e));
    }
    w->cap = capacity;
    w->ncols = h->L + h->nb_vars;
    return SDPCUT_OK;
}

int sdpcut_pool_destroy(sdpcut_handle h)
{
    if (!h) return SDPCUT_EINVAL;
    if (!h->pool) return SDPCUT_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sdpcut_sync(h));
    free_pool_ws(h);
    return SDPCUT_OK;
}

int sdpcut_pool_add_csr(sdpcut_handle h, int64_t n_rows, const int32_t *indptr, const int32_t *indices, const double *values,
                        const double *rhs, const int32_t *sense, int64_t *first_serial)
{
    if (!h) return SDPCUT_EINVAL;
    PoolWs *w = nullptr;
    int rc = pool_get_ws(h, &w);
    if (rc) return rc;
    SDPCUT_NO_PENDING(h);
    if (n_rows < 0) return sdpcut_fail(h, SDPCUT_EINVAL, "n_rows must be >= 0");
    if (first_serial) *first_serial = w->next_serial;
    if (n_rows == 0) return SDPCUT_OK;
    if (!indptr || !indices || !values || !rhs) return sdpcut_fail(h, SDPCUT_EINVAL, "bad pool_add_csr arguments");
    // every refusal comes before any state changes
    if (n_rows > w->cap - w->n) return sdpcut_fail(h, SDPCUT_EINVAL, "the block would exceed the pool's capacity");
    if (indptr[0] < 0) return sdpcut_fail(h, SDPCUT_EINVAL, "indptr must start at a non-negative offset");
    for (int64_t i = 0; i < n_rows; ++i) {
        const int64_t len = (int64_t)indptr[i + 1] - indptr[i];
        if (len < 1) return sdpcut_fail(h, SDPCUT_EINVAL, "a pool row must have at least one entry");
        if (len > POOL_LD) return sdpcut_fail(h, SDPCUT_EINVAL, "a pool row must have at most SDPCUT_ROW_LD entries");
        if (!std::isfinite(rhs[i])) return sdpcut_fail(h, SDPCUT_EINVAL, "a right-hand side is not finite");
        if (sense && sense[i] != 1 && sense[i] != -1) return sdpcut_fail(h, SDPCUT_EINVAL, "sense must be +1 (G) or -1 (L)");
    }
    const int64_t lo = indptr[0], nnz = (int64_t)indptr[n_rows] - lo;
    for (int64_t p = lo; p < lo + nnz; ++p) {
        if (indices[p] < 0 || indices[p] >= w->ncols) return sdpcut_fail(h, SDPCUT_EINVAL, "a column index lies outside the LP's columns");
        if (!std::isfinite(values[p])) return sdpcut_fail(h, SDPCUT_EINVAL, "a coefficient is not finite");
    }
    HIP_TRY(h, hipSetDevice(h->device));
    // the staged block: values | rhs | indptr (rebased to 0) | indices | sense
    const size_t o_val = 0, o_rhs = o_val + (size_t)nnz * 8, o_ptr = o_rhs + (size_t)n_rows * 8, o_ind = o_ptr + (size_t)(n_rows + 1) * 4,
                 o_sense = o_ind + (size_t)nnz * 4, bytes = o_sense + (size_t)n_rows * 4;
    rc = grow(h, w->stage, bytes);
    if (rc) return rc;
    char *s = (char *)w->stage.get();
    std::memcpy(s + o_val, values + lo, (size_t)nnz * 8);
    std::memcpy(s + o_rhs, rhs, (size_t)n_rows * 8);
    for (int64_t i = 0; i <= n_rows; ++i) ((int32_t *)(s + o_ptr))[i] = (int32_t)(indptr[i] - lo);
    std::memcpy(s + o_ind, indices + lo, (size_t)nnz * 4);
    for (int64_t i = 0; i < n_rows; ++i) ((int32_t *)(s + o_sense))[i] = sense ? sense[i] : 1;
    const char *d = (const char *)w->stage.dev();
    hipLaunchKernelGGL(pool_append_kernel, dim3(pool_grid(n_rows)), dim3(256), 0, h->stream, n_rows, w->n, w->cap, w->next_serial,
                       (const int32_t *)(d + o_ptr), (const int32_t *)(d + o_ind), (const double *)(d + o_val), (const double *)(d + o_rhs),
                       (const int32_t *)(d + o_sense), w->a[w->cur]);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, sdpcut_sync(h));      // the staging block is free again
    w->n += n_rows;
    w->n_lp += n_rows;
    w->next_serial += n_rows;
    return SDPCUT_OK;
}

int sdpcut_pool_step(sdpcut_handle h, const double *vars_values, const sdpcut_pool_params_t *params, sdpcut_pool_step_t *out)
{
    if (!h) return SDPCUT_EINVAL;
    if (!out) return sdpcut_fail(h, SDPCUT_EINVAL, "out is NULL");
    std::memset(out, 0, sizeof(*out));
    if (!params) return sdpcut_fail(h, SDPCUT_EINVAL, "params is NULL");
    if (!(params->tight_tol >= 0.0) || !std::isfinite(params->tight_tol) || !(params->viol_tol >= 0.0) || !std::isfinite(params->viol_tol))
        return sdpcut_fail(h, SDPCUT_EINVAL, "tight_tol and viol_tol must be finite and >= 0");
    if (params->max_age < 1 || params->drop_age < 1) return sdpcut_fail(h, SDPCUT_EINVAL, "max_age and drop_age must be >= 1");
    if (params->max_return < 0) return sdpcut_fail(h, SDPCUT_EINVAL, "max_return must be >= 0");
    PoolWs *w = nullptr;
    int rc = pool_get_ws(h, &w);
    if (rc) return rc;
    SDPCUT_NO_PENDING(h);
    if (!(h->have_point || vars_values)) return sdpcut_fail(h, SDPCUT_ESTATE, "a point first");
    if (vars_values && (rc = sdpcut_set_point(h, vars_values))) return rc;
    const int64_t n = w->n;
    out->n_in_lp = w->n_lp;
    out->n_parked = w->n_parked;
    if (n == 0) return SDPCUT_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const int64_t wmax = params->max_return < n ? params->max_return : n;
    const PoolOutLayout y = pool_out_layout(n, wmax);
    rc = grow(h, w->out, y.bytes);
    if (rc) return rc;
    if (wmax > 0 && (rc = ensure_rank_ws(h, n))) return rc;      // (may wait for the stream: before anything is enqueued)
    PoolArrays &a = w->a[w->cur], &b = w->a[1 - w->cur];
    const int g = pool_grid(n + 1);
    HIP_TRY(h, hipMemsetAsync(w->cnt.get(), 0, PC_WORDS * 8, h->stream));
    hipLaunchKernelGGL(pool_eval_kernel, dim3(g), dim3(256), 0, h->stream, n, w->cap, w->ncols, h->d_vars.get(), params->tight_tol,
                       params->viol_tol, params->max_age, a, w->key.get(), w->rowid.get(), w->mark.get(), w->cnt.get());
    HIP_TRY(h, hipGetLastError());
    if (wmax > 0) {
        // (key descending, row ascending) = (key descending, serial ascending): the rows are in ascending serial order
        rc = merge_topk_on_device(h, n, w->key.get(), nullptr, w->rowid.get(), wmax, w->key_out.get(), w->row_out.get());
        if (rc) return rc;
    }
    hipLaunchKernelGGL(pool_enter_kernel, dim3(pool_grid(wmax + 1)), dim3(256), 0, h->stream, wmax, n, w->row_out.get(), w->cnt.get(), a, w->mark.get(),
                       w->ennz.get());
    hipLaunchKernelGGL(pool_age_kernel, dim3(g), dim3(256), 0, h->stream, n, params->drop_age, a, w->mark.get(), w->flags.get(), w->cnt.get());
    HIP_TRY(h, hipGetLastError());
    size_t tb = w->scan_tmp.size();
    HIP_TRY(h, rocprim::exclusive_scan(w->scan_tmp.get(), tb, w->flags.get(), w->scan.get(), 0ull, (size_t)(n + 1), rocprim::plus<unsigned long long>(),
                                       h->stream));
    tb = w->scan_tmp.size();
    HIP_TRY(h, rocprim::exclusive_scan(w->scan_tmp.get(), tb, w->ennz.get(), w->eptr.get(), 0, (size_t)(wmax + 1), rocprim::plus<int32_t>(), h->stream));
    const int64_t lanes = n > wmax ? n : wmax;
    hipLaunchKernelGGL(pool_emit_kernel, dim3(pool_grid(lanes)), dim3(256), 0, h->stream, n, wmax, w->cap, a, w->mark.get(), w->scan.get(), w->row_out.get(),
                       w->key_out.get(), w->eptr.get(), w->cnt.get(), (char *)w->out.dev(), y);
    hipLaunchKernelGGL(pool_compact_kernel, dim3(g), dim3(256), 0, h->stream, n, w->cap, a, b, w->mark.get(), w->scan.get());
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, sdpcut_sync(h));      // the step's one host wait
    const char *blk = (const char *)w->out.get();
    const int64_t *hdr = (const int64_t *)blk;
    out->n_violated = hdr[0];
    out->n_leave = hdr[1];
    out->n_dropped = hdr[2];
    out->n_enter = hdr[3];
    out->enter_nnz = hdr[4];
    if (out->n_dropped > 0) w->cur = 1 - w->cur;
    w->n = n - out->n_dropped;
    w->n_lp += out->n_enter - out->n_leave;
    w->n_parked += out->n_leave - out->n_enter - out->n_dropped;
    out->n_in_lp = w->n_lp;
    out->n_parked = w->n_parked;
    out->leave = (const int64_t *)(blk + y.leave);
    out->dropped = (const int64_t *)(blk + y.dropped);
    out->enter = (const int64_t *)(blk + y.enter);
    out->enter_key = (const double *)(blk + y.key);
    out->enter_rhs = (const double *)(blk + y.rhs);
    out->enter_sense = (const int32_t *)(blk + y.sense);
    out->enter_indptr = (const int32_t *)(blk + y.indptr);
    out->enter_indices = (const int32_t *)(blk + y.indices);
    out->enter_values = (const double *)(blk + y.values);
    return SDPCUT_OK;
}

int sdpcut_pool_get(sdpcut_handle h, int64_t max_rows, int64_t *n_rows, int64_t *next_serial, int64_t *serial, int32_t *state,
                    int32_t *age, int32_t *nnz, int32_t *sense, double *rhs, double *norm, int32_t *cols, double *vals)
{
    if (!h) return SDPCUT_EINVAL;
    PoolWs *w = (PoolWs *)h->pool;
    if (!w) return sdpcut_fail(h, SDPCUT_ESTATE, "sdpcut_pool_create first");
    SDPCUT_NO_PENDING(h);
    if (n_rows) *n_rows = w->n;
    if (next_serial) *next_serial = w->next_serial;
    if (max_rows < 0) return sdpcut_fail(h, SDPCUT_EINVAL, "max_rows must be >= 0");
    const int64_t m = max_rows < w->n ? max_rows : w->n;
    if (m == 0) return SDPCUT_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sdpcut_sync(h));
    const PoolArrays &a = w->a[w->cur];
    const size_t mm = (size_t)m;
    if (serial) HIP_TRY(h, hipMemcpy(serial, a.serial, mm * 8, hipMemcpyDeviceToHost));
    if (state) HIP_TRY(h, hipMemcpy(state, a.state, mm * 4, hipMemcpyDeviceToHost));
    if (age) HIP_TRY(h, hipMemcpy(age, a.age, mm * 4, hipMemcpyDeviceToHost));
    if (nnz) HIP_TRY(h, hipMemcpy(nnz, a.nnz, mm * 4, hipMemcpyDeviceToHost));
    if (sense) HIP_TRY(h, hipMemcpy(sense, a.sense, mm * 4, hipMemcpyDeviceToHost));
    if (rhs) HIP_TRY(h, hipMemcpy(rhs, a.rhs, mm * 8, hipMemcpyDeviceToHost));
    if (norm) HIP_TRY(h, hipMemcpy(norm, a.norm, mm * 8, hipMemcpyDeviceToHost));
    if (cols || vals) {
        // slot-major on the device, row-major [m][SDPCUT_ROW_LD] for the caller
        std::vector<int32_t> tc(cols ? mm : 0);
        std::vector<double> tv(vals ? mm : 0);
        for (int s = 0; s < POOL_LD; ++s) {
            if (cols) {
                HIP_TRY(h, hipMemcpy(tc.data(), a.cols + (size_t)s * (size_t)w->cap, mm * 4, hipMemcpyDeviceToHost));
                for (size_t r = 0; r < mm; ++r) cols[r * POOL_LD + s] = tc[r];
            }
            if (vals) {
                HIP_TRY(h, hipMemcpy(tv.data(), a.vals + (size_t)s * (size_t)w->cap, mm * 8, hipMemcpyDeviceToHost));
                for (size_t r = 0; r < mm; ++r) vals[r * POOL_LD + s] = tv[r];
            }
        }
    }
    return SDPCUT_OK;
}

} // extern "C"
