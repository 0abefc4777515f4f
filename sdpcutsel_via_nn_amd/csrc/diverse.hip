// Diverse cut selection (include/sdpcut.h: sdpcut_round_csr_diverse, sdpcut_filter_parallel): a parallelism filter on the ranked
// head.  The ranking, the cut rows and the CSR assembly are the existing ones (sdpcut_rank_device, cut_rows_kernel, round_csr_kernel);
// new here are the three steps between them:
//   div_prepare_kernel  one lane per pool entry: norm of its row, eligibility, its index set
//   div_pairs_kernel    one bit per pair s < t of the pool: |<a_s, a_t>| > max_parallel |a_s| |a_t|  (lower-triangular bit matrix)
//   div_greedy_kernel   ONE workgroup walks the pool in rank order, 64 entries at a time, accepted mask in LDS
// and, for a batch of LP points (sdpcut_round_csr_points_diverse), the three in one kernel with a workgroup per point:
//   div_rows_points_kernel / div_points_kernel   pools of at most 512 entries, rows, bits and sets in LDS
// The walk is the definition of DESIGN.md section 5 "Diverse selection"; diversity.py is its numpy twin.
#include <cstring>
#include <new>

#include "common.h"
#include "rows_dev.h"

#define DIV_MAX_POOL SDPCUT_DIVERSE_MAX_POOL
#define DIV_WORDS (DIV_MAX_POOL / 64)

// everything the filter keeps on the device, sized for `cap` pool entries (grown on demand, freed with the handle)
struct DiverseWs {
    DevBuf<int64_t> ids;       // [cap] candidate ids of the pool in rank order (global for a ranked pool, local for a caller's list)
    DevBuf<double> score;      // [cap]
    DevBuf<double> lam, rhs, norm;   // [cap]
    DevBuf<double> coef;       // [cap][SDPCUT_ROW_LD]
    DevBuf<int32_t> ks;        // [cap]
    DevBuf<int32_t> sets;      // [cap][5] padded with -1
    DevBuf<uint8_t> elig;      // [cap]
    DevBuf<uint8_t> keep;      // [cap]
    DevBuf<int64_t> acc_ids;   // [cap] accepted entries, compacted in rank order: the head the CSR assembly reads
    DevBuf<double> acc_score;  // [cap]
    DevBuf<int64_t> info;      // [8]: examined, skipped (not eligible), rejected (parallel), accepted, 0, 0, 0; kept when the others grow
    DevBuf<unsigned long long> bits;   // lower-triangular bit matrix, see div_bits_offset; grows on its own
};

// Rows 64 b .. 64 b + 63 of the bit matrix hold b + 1 words each (columns 0 .. 64 b + 63); the blocks follow one another.
// 16384 entries: 64 * 256 * 257 / 2 words = 16.8 MB.
static __host__ __device__ __forceinline__ int64_t div_bits_offset(int64_t t)
{
    const int64_t b = t >> 6;
    return 32 * b * (b + 1) + (t & 63) * (b + 1);
}
static inline int64_t div_bits_words(int64_t blocks) { return 32 * blocks * (blocks + 1); }

void free_diverse_ws(sdpcut_ctx *h)
{
    delete (DiverseWs *)h->diverse;
    h->diverse = nullptr;
}

// workspace for a pool of P entries; with_bits: the pair test will run (max_parallel < 1)
static int div_ensure(sdpcut_ctx *h, int64_t P, bool with_bits, DiverseWs **out)
{
    DiverseWs *w = (DiverseWs *)h->diverse;
    if (!w) {
        w = new (std::nothrow) DiverseWs();
        if (!w) return sdpcut_fail(h, SDPCUT_ENOMEM, "out of host memory");
        h->diverse = w;
    }
    int rc;
    if ((rc = grow(h, w->info, 8))) return rc;
    // the twelve arrays of the pool are all asked for c entries, a multiple of 64: they grow together
    const size_t c = (size_t)((P + 63) & ~(int64_t)63);
    if ((rc = grow(h, w->ids, c)) || (rc = grow(h, w->score, c)) || (rc = grow(h, w->lam, c)) || (rc = grow(h, w->rhs, c)) ||
        (rc = grow(h, w->norm, c)) || (rc = grow(h, w->coef, c * SDPCUT_ROW_LD)) || (rc = grow(h, w->ks, c)) || (rc = grow(h, w->sets, c * 5)) ||
        (rc = grow(h, w->elig, c)) || (rc = grow(h, w->keep, c)) || (rc = grow(h, w->acc_ids, c)) || (rc = grow(h, w->acc_score, c)))
        return rc;
    if (with_bits && (rc = grow(h, w->bits, (size_t)div_bits_words((P + 63) / 64)))) return rc;
    *out = w;
    return 0;
}

// ------------------------------------------------------------------------------------------
// Norm, eligibility and index set of every pool entry; the rows themselves are cut_rows_kernel's (rows.hip), stride SDPCUT_ROW_LD,
// zero beyond the row's length.  An id outside the list has ks = 0 there and is not eligible.
__global__ __launch_bounds__(64) void div_prepare_kernel(int64_t P, const int64_t *ids, int64_t idx_base, int64_t n_local,
                                                         const int32_t *set5, const double *lam, const double *coef, const int32_t *ks,
                                                         double *norm, uint8_t *elig, int32_t *sets)
{
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= P) return;
    const int k = ks[t];
    const int64_t c = ids[t] - idx_base;
    const bool in_list = c >= 0 && c < n_local && k >= 2 && k <= SDPCUT_MAX_K;
    double ss = 0.0;
    {
#pragma clang fp contract(off)
        for (int m = 0; m < SDPCUT_ROW_LD; ++m) {
            const double v = coef[t * SDPCUT_ROW_LD + m];
            ss = ss + v * v;
        }
    }
    const double nr = in_list ? sqrt(ss) : 0.0;
    norm[t] = nr;
    elig[t] = (in_list && lam[t] < SDPCUT_NEG_EIGVAL && nr > 0.0) ? 1 : 0;
    for (int a = 0; a < 5; ++a) sets[t * 5 + a] = (in_list && a < k) ? set5[c * 5 + a] : -1;
}

// <a_s, a_t> over the shared LP columns: x_c for every common variable c, X_cd for common c <= d.  m[a] = position in s's set of
// t's a-th variable (-1: not shared).  Coefficient positions: a for x of local index a, k + a k - a (a - 1) / 2 + (b - a) for X of
// the local pair a <= b.  Fixed order: the x columns by t's ascending local index, then the X pairs row-major; no contraction.
// ct / cs: rows in LDS (their positions depend on the candidate sizes).
__device__ __forceinline__ double div_dot(const double *ct, int kt, const double *cs, int ks, const int (&m)[5])
{
#pragma clang fp contract(off)
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 5; ++a)
        if (m[a] >= 0) acc = acc + ct[a] * cs[m[a]];
#pragma unroll
    for (int a = 0; a < 5; ++a) {
#pragma unroll
        for (int b = a; b < 5; ++b) {
            if (m[a] < 0 || m[b] < 0) continue;
            const int pa = m[a] < m[b] ? m[a] : m[b], pb = m[a] < m[b] ? m[b] : m[a];
            acc = acc + ct[kt + a * kt - a * (a - 1) / 2 + (b - a)] * cs[ks + pa * ks - pa * (pa - 1) / 2 + (pb - pa)];
        }
    }
    return acc;
}

// Tile (row block blockIdx.y, column word blockIdx.x <= blockIdx.y) of the bit matrix: lane l owns row t = 64 by + l and tests
// it against the 64 entries s of the column word; both sets of rows sit in LDS.  A lane's 64 results leave as ONE word, stored by
// that lane.
__global__ __launch_bounds__(64) void div_pairs_kernel(int64_t P, double max_parallel, const double *coef, const int32_t *ks,
                                                       const int32_t *sets, const double *norm, const uint8_t *elig,
                                                       unsigned long long *bits)
{
    const int bx = blockIdx.x, by = blockIdx.y;
    if (bx > by) return;
    __shared__ double s_coef[64 * SDPCUT_ROW_LD];
    __shared__ double t_coef[64 * SDPCUT_ROW_LD];
    __shared__ double s_norm[64];
    __shared__ int32_t s_set[64 * 5];
    __shared__ int32_t s_k[64];
    __shared__ int32_t s_el[64];
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)by * 64 + lane;
    {
        const int64_t s = (int64_t)bx * 64 + lane;
        const bool live = s < P;
        s_norm[lane] = live ? norm[s] : 0.0;
        s_k[lane] = live ? ks[s] : 0;
        s_el[lane] = live ? (int32_t)elig[s] : 0;
        for (int a = 0; a < 5; ++a) s_set[lane * 5 + a] = live ? sets[s * 5 + a] : -1;
        for (int m = 0; m < SDPCUT_ROW_LD; ++m) {
            s_coef[lane * SDPCUT_ROW_LD + m] = live ? coef[s * SDPCUT_ROW_LD + m] : 0.0;
            t_coef[lane * SDPCUT_ROW_LD + m] = t < P ? coef[t * SDPCUT_ROW_LD + m] : 0.0;
        }
    }
    __syncthreads();
    if (t >= P) return;
    unsigned long long word = 0ull;
    if (elig[t]) {
        int32_t st[5];
#pragma unroll
        for (int a = 0; a < 5; ++a) st[a] = sets[t * 5 + a];      // -1 beyond the candidate's size: matches nothing
        const double *ct = t_coef + lane * SDPCUT_ROW_LD;
        const int kt = ks[t];
        const double nt = norm[t];
        const int jmax = (bx == by) ? lane : 64;      // pairs s < t only
        for (int j = 0; j < jmax; ++j) {
            if (!s_el[j]) continue;
            const int kj = s_k[j];
            int m[5];
            bool any = false;
#pragma unroll
            for (int a = 0; a < 5; ++a) {
                m[a] = -1;
#pragma unroll
                for (int b = 0; b < 5; ++b)
                    if (st[a] >= 0 && s_set[j * 5 + b] == st[a]) m[a] = b;
                any = any || m[a] >= 0;
            }
            if (!any) continue;       // no common variable, no common column
            const double dot = div_dot(ct, kt, s_coef + j * SDPCUT_ROW_LD, kj, m);
            bool hit;
            {
#pragma clang fp contract(off)
                hit = fabs(dot) > max_parallel * s_norm[j] * nt;
            }
            if (hit) word |= 1ull << j;
        }
    }
    bits[div_bits_offset(t) + bx] = word;
}

// The walk.  One workgroup of 256 threads; block b = entries 64 b .. 64 b + 63.  (1) Four threads per entry AND its row of the bit
// matrix against the accepted mask of the blocks in front (LDS); (2) the first wave settles the block's own entries one after the other from
// the in-block word of each (bits s < t of the diagonal tile); (3) lanes store keep flags and the compacted head.  The walk ends with
// the entry that fills the quota.  bits == NULL: no comparison at all (max_parallel >= 1).
__global__ __launch_bounds__(256) void div_greedy_kernel(int64_t P, int64_t quota, const uint8_t *elig, const unsigned long long *bits,
                                                         const int64_t *ids, const double *score, uint8_t *keep, int64_t *acc_ids,
                                                         double *acc_score, int64_t *info)
{
    __shared__ unsigned long long s_acc[DIV_WORDS];
    __shared__ unsigned long long s_diag[64];
    __shared__ int32_t s_conf[256];
    __shared__ int32_t s_el[64];
    __shared__ unsigned long long s_word;
    __shared__ int64_t s_cnt[4];      // accepted, examined, skipped, rejected
    const int tid = threadIdx.x;
    const int l = tid & 63, q = tid >> 6;
    if (tid < 4) s_cnt[tid] = 0;
    const int64_t nblk = (P + 63) / 64;
    __syncthreads();
    for (int64_t b = 0; b < nblk; ++b) {
        const int64_t t = b * 64 + l;
        const bool live = t < P;
        int conf = 0;
        if (bits && live && elig[t]) {
            const unsigned long long *row = bits + div_bits_offset(t);
            for (int64_t w = q; w < b; w += 4) {
                const unsigned long long a = s_acc[w];
                if (a && (row[w] & a)) conf = 1;
            }
            if (q == 0) s_diag[l] = row[b];
        } else if (q == 0) {
            s_diag[l] = 0ull;
        }
        if (q == 0) s_el[l] = (live && elig[t]) ? 1 : 0;
        s_conf[tid] = conf;
        __syncthreads();
        if (q == 0) {
            // the whole first wave, every lane with its own entry in registers: entry j is accepted iff it is eligible, clear of
            // the blocks in front and clear of what this block has accepted so far -- lane j's bit of the ballot in step j
            const bool ok = s_el[l] && !(s_conf[l] | s_conf[64 + l] | s_conf[128 + l] | s_conf[192 + l]);
            const unsigned long long d = s_diag[l];
            unsigned long long acc = 0ull;
            int64_t n_acc = s_cnt[0];
            const int nlive = (P - b * 64 < 64) ? (int)(P - b * 64) : 64;
            int j = 0;
            for (; j < nlive && n_acc < quota; ++j) {
                const unsigned long long m = __ballot(ok && !(d & acc));
                if ((m >> j) & 1ull) { acc |= 1ull << j; ++n_acc; }
            }
            // (the walk ends WITH the entry that fills the quota: what follows it in the block was not examined)
            const unsigned long long seen = j >= 64 ? ~0ull : ((1ull << j) - 1ull);
            const unsigned long long el = __ballot(s_el[l] != 0);
            if (l == 0) {
                s_word = acc;
                s_acc[b] = acc;
                s_cnt[1] += j;
                s_cnt[2] += __popcll(~el & seen);
                s_cnt[3] += __popcll(el & seen & ~acc);
                // s_cnt[0] is advanced after the lanes have read it as their base
            }
        }
        __syncthreads();
        const unsigned long long acc = s_word;
        const int64_t base = s_cnt[0];
        if (q == 0 && live) {
            const bool mine = (acc >> l) & 1ull;
            keep[t] = mine ? 1 : 0;
            if (mine) {
                const int64_t pos = base + __popcll(acc & ((1ull << l) - 1ull));
                acc_ids[pos] = ids[t];
                acc_score[pos] = score[t];
            }
        }
        __syncthreads();
        if (tid == 0) s_cnt[0] = base + __popcll(acc);
        __syncthreads();
        if (s_cnt[0] >= quota) {
            // entries behind the walk's end keep nothing
            for (int64_t r = (b + 1) * 64 + tid; r < P; r += 256) keep[r] = 0;
            break;
        }
    }
    __syncthreads();
    if (tid == 0) {
        info[0] = s_cnt[1];
        info[1] = s_cnt[2];
        info[2] = s_cnt[3];
        info[3] = s_cnt[0];
        info[4] = info[5] = info[6] = info[7] = 0;
    }
}

// ------------------------------------------------------------------------------------------
// rows -> norms -> pair bits -> walk, for the P ids in w->ids (minus idx_base = local candidate index); all on the handle's stream
static int div_filter_enqueue(sdpcut_ctx *h, DiverseWs *w, int64_t P, int64_t idx_base, int64_t quota, double max_parallel)
{
    int rc = launch_cut_rows(h, P, nullptr, w->ids.get(), idx_base, w->lam.get(), w->coef.get(), SDPCUT_ROW_LD, w->rhs.get(), nullptr, w->ks.get());
    if (rc) return rc;
    const int grid = (int)((P + 63) / 64);
    hipLaunchKernelGGL(div_prepare_kernel, dim3(grid), dim3(64), 0, h->stream, P, w->ids.get(), idx_base, h->N, h->d_set_orig.get(), w->lam.get(), w->coef.get(),
                       w->ks.get(), w->norm.get(), w->elig.get(), w->sets.get());
    HIP_TRY(h, hipGetLastError());
    const bool compare = max_parallel < 1.0;
    if (compare) {
        hipLaunchKernelGGL(div_pairs_kernel, dim3(grid, grid), dim3(64), 0, h->stream, P, max_parallel, w->coef.get(), w->ks.get(), w->sets.get(), w->norm.get(),
                           w->elig.get(), w->bits.get());
        HIP_TRY(h, hipGetLastError());
    }
    hipLaunchKernelGGL(div_greedy_kernel, dim3(1), dim3(256), 0, h->stream, P, quota, w->elig.get(), compare ? w->bits.get() : nullptr, w->ids.get(),
                       w->score.get(), w->keep.get(), w->acc_ids.get(), w->acc_score.get(), w->info.get());
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------
// The filter over a batch of LP points (sdpcut_round_csr_points_diverse, points.hip): the same three steps, ONE workgroup per
// point, everything between the pool's rows and the accepted head in LDS.  No workgroup reads what another writes.

// Row y of the grid: the rows of the pool of point y, as cut_rows_kernel writes them (stride SDPCUT_ROW_LD, zero beyond the row's
// length), built with the lambda_min the point's score row holds (eig NULL: the row computes it).  The pool's length is what the
// point's selection left in its counters (k_eff; a void selection has no pool).
__global__ __launch_bounds__(64) void div_rows_points_kernel(DivPointsArgs A)
{
    const int64_t p = blockIdx.y;
    const int64_t *c4 = A.sel_c4 + p * A.c4_stride;
    int64_t P = c4[4] ? 0 : c4[3];
    if (P > A.pool) P = A.pool;
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= P) return;
    const int64_t e = p * A.pool + t;
    const int64_t c = A.idx[e] - A.idx_base;
    double co[SDPCUT_ROW_LD];
    int64_t cl[SDPCUT_ROW_LD];
#pragma unroll
    for (int m = 0; m < SDPCUT_ROW_LD; ++m) { co[m] = 0.0; cl[m] = -1; }
    double lam = __builtin_nan(""), rhs = 0.0;
    int k = 0;
    if (c >= 0 && c < A.n_local) {
        k = A.ks[c];
        const int32_t *s5 = A.set5 + c * 5;
        CALL_FOR_SET_SIZE(k, cut_row_one, s5, A.vars + p * A.vars_ld, A.nv, A.L, &lam, co, &rhs, cl, A.eig ? A.eig + p * A.eig_ld + c : nullptr);
    }
    A.row_ks[e] = k;
    A.row_lam[e] = lam;
#pragma unroll
    for (int m = 0; m < SDPCUT_ROW_LD; ++m) A.row_coef[e * SDPCUT_ROW_LD + m] = co[m];
}

// Workgroup p filters the pool of point p.  (1) rows -> LDS; (2) norm, eligibility, index set of every entry as
// div_prepare_kernel; (3) the lower-triangular pair bits as div_pairs_kernel, tile (row block, column word) by tile, the tiles dealt
// to the eight waves in turn; (4) the walk of div_greedy_kernel, eight threads per entry over the words in front; (5) the accepted
// entries compacted in rank order into the point's head row, the walk's counts into info[p] (the selection counters of the row
// assembly: word 3 = accepted) and the selection's own counters to the host.  compare == 0 (max_parallel >= 1): no (3), no bit
// is read.  LDS: rows 80 KB + bits 18 KB + sets 10 KB + norms, sizes, flags 8 KB + the walk's words.
__global__ __launch_bounds__(DIVP_THREADS) void div_points_kernel(DivPointsArgs A)
{
    __shared__ double s_coef[DIVP_MAX_POOL * SDPCUT_ROW_LD];
    __shared__ unsigned long long s_bits[32 * (DIVP_MAX_POOL / 64) * (DIVP_MAX_POOL / 64 + 1)];
    __shared__ int32_t s_set[DIVP_MAX_POOL * 5];
    __shared__ double s_norm[DIVP_MAX_POOL];
    __shared__ int32_t s_k[DIVP_MAX_POOL];
    __shared__ int32_t s_elig[DIVP_MAX_POOL];
    __shared__ unsigned long long s_acc[DIVP_MAX_POOL / 64];
    __shared__ unsigned long long s_diag[64];
    __shared__ int32_t s_conf[DIVP_THREADS];
    __shared__ unsigned long long s_word;
    __shared__ int64_t s_cnt[4];      // accepted, examined, skipped, rejected
    const int tid = threadIdx.x;
    const int l = tid & 63, q = tid >> 6;
    const int64_t p = blockIdx.x;
    const int64_t *c4 = A.sel_c4 + p * A.c4_stride;
    int P = c4[4] ? 0 : (int)(c4[3] < A.pool ? c4[3] : A.pool);      // (uniform)
    if (tid < 8) A.sel_out[p * 8 + tid] = tid < 7 ? c4[tid] : 0;
    const int64_t *ids = A.idx + p * A.pool;
    const double *score = A.score + p * A.pool;
    if (tid < 4) s_cnt[tid] = 0;
    // (1), (2)
    {
        const double *g = A.row_coef + p * A.pool * SDPCUT_ROW_LD;
        for (int i = tid; i < P * SDPCUT_ROW_LD; i += DIVP_THREADS) s_coef[i] = g[i];
    }
    __syncthreads();
    for (int t = tid; t < DIVP_MAX_POOL; t += DIVP_THREADS) {
        double nr = 0.0;
        int el = 0, k = 0;
        int64_t c = -1;
        bool in_list = false;
        if (t < P) {
            k = A.row_ks[p * A.pool + t];
            c = ids[t] - A.idx_base;
            in_list = c >= 0 && c < A.n_local && k >= 2 && k <= SDPCUT_MAX_K;
            double ss = 0.0;
            {
#pragma clang fp contract(off)
                for (int m = 0; m < SDPCUT_ROW_LD; ++m) {
                    const double v = s_coef[t * SDPCUT_ROW_LD + m];
                    ss = ss + v * v;
                }
            }
            nr = in_list ? sqrt(ss) : 0.0;
            el = (in_list && A.row_lam[p * A.pool + t] < SDPCUT_NEG_EIGVAL && nr > 0.0) ? 1 : 0;
        }
        s_norm[t] = nr;
        s_k[t] = k;
        s_elig[t] = el;
        for (int a = 0; a < 5; ++a) s_set[t * 5 + a] = (in_list && a < k) ? A.set5[c * 5 + a] : -1;
    }
    __syncthreads();
    const int nblk = (P + 63) / 64;
    // (3)
    if (A.compare) {
        int tile = 0;
        for (int by = 0; by < nblk; ++by) {
            for (int bx = 0; bx <= by; ++bx, ++tile) {
                if ((tile & (DIVP_THREADS / 64 - 1)) != q) continue;      // (uniform in the wave)
                const int t = by * 64 + l;
                if (t >= P) continue;
                unsigned long long word = 0ull;
                if (s_elig[t]) {
                    int32_t st[5];
#pragma unroll
                    for (int a = 0; a < 5; ++a) st[a] = s_set[t * 5 + a];
                    const double *ct = s_coef + t * SDPCUT_ROW_LD;
                    const int kt = s_k[t];
                    const double nt = s_norm[t];
                    const int jmax = (bx == by) ? l : 64;      // pairs s < t only
                    for (int j = 0; j < jmax; ++j) {
                        const int s = bx * 64 + j;
                        if (!s_elig[s]) continue;
                        const int kj = s_k[s];
                        int m[5];
                        bool any = false;
#pragma unroll
                        for (int a = 0; a < 5; ++a) {
                            m[a] = -1;
#pragma unroll
                            for (int b = 0; b < 5; ++b)
                                if (st[a] >= 0 && s_set[s * 5 + b] == st[a]) m[a] = b;
                            any = any || m[a] >= 0;
                        }
                        if (!any) continue;
                        const double dot = div_dot(ct, kt, s_coef + s * SDPCUT_ROW_LD, kj, m);
                        bool hit;
                        {
#pragma clang fp contract(off)
                            hit = fabs(dot) > A.max_parallel * s_norm[s] * nt;
                        }
                        if (hit) word |= 1ull << j;
                    }
                }
                s_bits[div_bits_offset(t) + bx] = word;
            }
        }
    }
    __syncthreads();
    // (4), (5)
    int64_t *acc_ids = A.acc_idx + p * A.cap;
    double *acc_score = A.acc_score + p * A.cap;
    for (int b = 0; b < nblk; ++b) {
        const int t = b * 64 + l;
        const bool live = t < P;
        int conf = 0;
        if (A.compare && live && s_elig[t]) {
            const unsigned long long *row = s_bits + div_bits_offset(t);
            for (int w = q; w < b; w += DIVP_THREADS / 64) {
                const unsigned long long a = s_acc[w];
                if (a && (row[w] & a)) conf = 1;
            }
            if (q == 0) s_diag[l] = row[b];
        } else if (q == 0) {
            s_diag[l] = 0ull;
        }
        s_conf[tid] = conf;
        __syncthreads();
        if (q == 0) {
            int cf = 0;
#pragma unroll
            for (int w = 0; w < DIVP_THREADS / 64; ++w) cf |= s_conf[w * 64 + l];
            const bool el = live && s_elig[t];
            const bool ok = el && !cf;
            const unsigned long long d = s_diag[l];
            unsigned long long acc = 0ull;
            int64_t n_acc = s_cnt[0];
            const int nlive = (P - b * 64 < 64) ? (P - b * 64) : 64;
            int j = 0;
            for (; j < nlive && n_acc < A.quota; ++j) {
                const unsigned long long m = __ballot(ok && !(d & acc));
                if ((m >> j) & 1ull) { acc |= 1ull << j; ++n_acc; }
            }
            // (the walk ends WITH the entry that fills the quota: what follows it in the block was not examined)
            const unsigned long long seen = j >= 64 ? ~0ull : ((1ull << j) - 1ull);
            const unsigned long long elm = __ballot(el);
            if (l == 0) {
                s_word = acc;
                s_acc[b] = acc;
                s_cnt[1] += j;
                s_cnt[2] += __popcll(~elm & seen);
                s_cnt[3] += __popcll(elm & seen & ~acc);
            }
        }
        __syncthreads();
        const unsigned long long acc = s_word;
        const int64_t base = s_cnt[0];
        if (q == 0 && live && ((acc >> l) & 1ull)) {
            const int64_t pos = base + __popcll(acc & ((1ull << l) - 1ull));
            acc_ids[pos] = ids[t];
            acc_score[pos] = score[t];
        }
        __syncthreads();
        if (tid == 0) s_cnt[0] = base + __popcll(acc);
        __syncthreads();
        if (s_cnt[0] >= A.quota) break;
    }
    __syncthreads();
    if (tid == 0) {
        int64_t *info = A.info + p * 8;
        info[0] = s_cnt[1];
        info[1] = s_cnt[2];
        info[2] = s_cnt[3];
        info[3] = s_cnt[0];
        info[4] = info[5] = info[6] = info[7] = 0;
    }
}

int launch_div_points(sdpcut_ctx *h, int n_points, const DivPointsArgs &A)
{
    if (n_points <= 0) return 0;
    if (A.pool < 1 || A.pool > DIVP_MAX_POOL || A.cap < 1 || A.cap > A.pool) return sdpcut_fail(h, SDPCUT_EINVAL, "div_points: pool out of range");
    hipLaunchKernelGGL(div_rows_points_kernel, dim3((unsigned)((A.pool + 63) / 64), (unsigned)n_points), dim3(64), 0, h->stream, A);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(div_points_kernel, dim3((unsigned)n_points), dim3(DIVP_THREADS), 0, h->stream, A);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

static int div_check_common(sdpcut_ctx *h, double max_parallel)
{
    if (!(max_parallel >= 0.0 && max_parallel <= 1.0)) return sdpcut_fail(h, SDPCUT_EINVAL, "max_parallel must lie in [0, 1]");
    return 0;
}

extern "C" {

int sdpcut_filter_parallel(sdpcut_handle h, int64_t count, const int64_t *idx, int64_t quota, double max_parallel, uint8_t *keep_out,
                           sdpcut_diverse_info_t *info)
{
    if (!h) return SDPCUT_EINVAL;
    int rc = div_check_common(h, max_parallel);
    if (rc) return rc;
    if (count < 0 || count > DIV_MAX_POOL) return sdpcut_fail(h, SDPCUT_EINVAL, "count must lie in 0 .. SDPCUT_DIVERSE_MAX_POOL");
    if (quota < 1) return sdpcut_fail(h, SDPCUT_EINVAL, "quota must be >= 1");
    if (count > 0 && (!idx || !keep_out)) return sdpcut_fail(h, SDPCUT_EINVAL, "bad filter_parallel arguments");
    if (!h->have_point || !h->d_set_orig.get()) return sdpcut_fail(h, SDPCUT_ESTATE, "set_candidates and set_point first");
    SDPCUT_NO_PENDING(h);
    for (int64_t i = 0; i < count; ++i)
        if (idx[i] < 0 || idx[i] >= h->N) return sdpcut_fail(h, SDPCUT_EINVAL, "candidate index out of range");
    if (info) { info->pool = count; info->examined = info->skipped_nonviolated = info->rejected_parallel = 0; }
    if (count == 0) return SDPCUT_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    DiverseWs *w = nullptr;
    rc = div_ensure(h, count, max_parallel < 1.0, &w);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(w->ids.get(), idx, (size_t)count * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(w->score.get(), 0, (size_t)count * 8, h->stream));
    rc = div_filter_enqueue(h, w, count, 0, quota, max_parallel);
    if (rc) return rc;
    int64_t c8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(h, hipMemcpyAsync(keep_out, w->keep.get(), (size_t)count, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(c8, w->info.get(), sizeof(c8), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    if (info) { info->examined = c8[0]; info->skipped_nonviolated = c8[1]; info->rejected_parallel = c8[2]; }
    return SDPCUT_OK;
}

int sdpcut_round_csr_diverse(sdpcut_handle h, const double *vars_values, int strat, int64_t sel_size, int64_t pool_size,
                             double max_parallel, sdpcut_round_csr_t *out, sdpcut_diverse_info_t *info)
{
    if (!h) return SDPCUT_EINVAL;
    if (!out) return sdpcut_fail(h, SDPCUT_EINVAL, "out is NULL");
    std::memset(out, 0, sizeof(*out));
    if (info) std::memset(info, 0, sizeof(*info));
    int rc;
    const bool by_eff = strat == SDPCUT_STRAT_EFF;      // ranks through a view inside the ranking calls (common.h: MeasureAsObj)
    if (!by_eff && (rc = check_round_strategy(h, strat))) return rc;
    rc = div_check_common(h, max_parallel);
    if (rc) return rc;
    if (sel_size < 1) return sdpcut_fail(h, SDPCUT_EINVAL, "sel_size must be >= 1");
    if (pool_size < sel_size) return sdpcut_fail(h, SDPCUT_EINVAL, "pool_size must be >= sel_size");
    if (pool_size > DIV_MAX_POOL) return sdpcut_fail(h, SDPCUT_EINVAL, "pool_size must not exceed SDPCUT_DIVERSE_MAX_POOL");
    if (h->nb_vars == 0 || !h->d_eig.get() || !(h->have_point || vars_values))
        return sdpcut_fail(h, SDPCUT_ESTATE, "set_instance, set_candidates and a point first");
    SDPCUT_NO_PENDING(h);
    if (vars_values && (rc = sdpcut_set_point(h, vars_values))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    // 1. the pool: the head of the strategy's ranking, by the existing ranking call (SDPCUT_OPT_EXACT_HEAD included)
    const uint32_t need = by_eff ? (uint32_t)SDPCUT_EFF : strat_need(strat);
    if ((rc = obj_complete(h))) return rc;      // a measure a skipped round left partial: whole before this round counts by it
    if ((h->scored & need) != need && (rc = sdpcut_score(h, need & ~h->scored))) return rc;
    const int64_t want = pool_size < h->N ? pool_size : h->N;
    out->row_ld = h->row_len_max;
    if (want == 0) return sdpcut_rank(h, strat, sel_size, 0, nullptr, nullptr, &out->n_total, &out->new_strat, out->counters);
    DiverseWs *w = nullptr;
    rc = div_ensure(h, want, max_parallel < 1.0, &w);
    if (rc) return rc;
    int64_t P = 0;
    rc = sdpcut_rank_device(h, strat, sel_size, want, w->ids.get(), w->score.get(), &P, &out->n_total, &out->new_strat, out->counters);
    if (rc) return rc;
    if (info) info->pool = P;
    if (P <= 0) return SDPCUT_OK;      // an empty ranking (no violated candidate): an empty block
    // 2. - 4. rows, pair test, walk
    rc = div_filter_enqueue(h, w, P, h->base, sel_size, max_parallel);
    if (rc) return rc;
    // 5. emit: the accepted entries are a head like any other; the existing assembly reads its length from word 3 of w->info and
    // copies the walk's counts into the block's header with it
    const int64_t cap = sel_size < P ? sel_size : P;
    const int32_t ld = h->row_len_max;
    rc = ensure_pinned(h, csr_layout(cap, ld).bytes);
    if (rc) return rc;
    const int64_t *hdr = (const int64_t *)h->pinned.get();
    rc = csr_assemble_wait(h, 10, 2, true, "round_csr_diverse", [&](int64_t serial) {
        return launch_round_csr(h, cap, w->info.get(), cap, w->acc_ids.get(), w->acc_score.get(), ld, h->pinned.dev(), serial);
    });
    if (rc) return rc;
    ++h->stat_rounds;
    if (info) { info->examined = hdr[0]; info->skipped_nonviolated = hdr[1]; info->rejected_parallel = hdr[2]; }
    out->cap = cap;
    out->n_out = hdr[3];
    csr_out_from_block(h->pinned.get(), out);
    return SDPCUT_OK;
}

} // extern "C"
