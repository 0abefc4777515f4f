// Epilogues of a selection round: the eigen-cut rows of the selected candidates
// (cut_select_qp.py:737-750) -- as padded rows (cut_rows_kernel, round_rows_kernel) or assembled into
// one CSR block on the device (round_csr_kernel: SURVEY 8 f row 4, the replacement of the per-cut
// SparsePair loop of :747-754) -- written straight into pinned host memory, and the LP point's way in.
// The gather, the row of an eigenvector, the look-back and the completion word are rows_dev.h's, shared with the multi-cut
// kernels (multirows.hip); the completion ticket and the look-back words of a handle are allocated here (ensure_round_sync).
#include <hip/hip_ext.h>

#include "common.h"
#include "rows_dev.h"
#include "topk_dev.h"

// ------------------------------------------------------------------------------------------
// Eigen-cut rows of selected candidates (cut_select_qp.py:737-750), one lane per cut: cut_row_one of rows_dev.h.

// count may be an upper bound: if d_limit != NULL only min(count, *d_limit) rows exist (the
// device-side length of a ranking that the host has not read yet).  coef rows have stride
// coef_ld >= k + k(k+1)/2 of the largest candidate; cols (stride SDPCUT_ROW_LD) is optional.
__global__ __launch_bounds__(64) void cut_rows_kernel(int64_t count, const int64_t *d_limit, const int64_t *idx,
                                                      int64_t idx_base, int64_t n_local, const int32_t *set5,
                                                      const int32_t *ks,
                                                      const double *vars, int32_t nv, int64_t L, double *lam,
                                                      double *coef, int coef_ld, double *rhs, int64_t *cols,
                                                      int32_t *ks_out, const double *eig)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (d_limit && *d_limit < count) count = *d_limit;
    if (i >= count) return;
    const int64_t c = idx[i] - idx_base;
    if (c < 0 || c >= n_local) {   // a candidate of another shard (sdpcut_shard_finish_round): no row here
        ks_out[i] = 0;
        lam[i] = __builtin_nan("");
        rhs[i] = 0.0;
        for (int m = 0; m < coef_ld; ++m) coef[i * coef_ld + m] = 0.0;
        if (cols)
            for (int m = 0; m < SDPCUT_ROW_LD; ++m) cols[i * SDPCUT_ROW_LD + m] = -1;
        return;
    }
    const int k = ks[c];
    const int32_t *s5 = set5 + c * 5;
    double co[SDPCUT_ROW_LD];
    int64_t cl[SDPCUT_ROW_LD];
#pragma unroll
    for (int m = 0; m < SDPCUT_ROW_LD; ++m) { co[m] = 0.0; cl[m] = -1; }
    ks_out[i] = k;
    CALL_FOR_SET_SIZE(k, cut_row_one, s5, vars, nv, L, lam + i, co, rhs + i, cl, eig ? eig + c : nullptr);
#pragma unroll
    for (int m = 0; m < SDPCUT_ROW_LD; ++m) {
        if (m < coef_ld) coef[i * coef_ld + m] = co[m];
        if (cols) cols[i * SDPCUT_ROW_LD + m] = cl[m];
    }
}

// Epilogue of a fused round (sdpcut_select_round): the rows of the ranking head together with
// its ids, scores and the four ranking counters go straight into the caller-visible block --
// pinned host memory mapped into the device, so the stores ARE the device-to-host transfer (no
// SDMA hand-off, no extra copy launch).  Layout (cap entries): 64 B counters | idx | score | lam |
// rhs | coef [cap][coef_ld] | ks.  Coefficient rows are staged in LDS and leave as contiguous
// coalesced stores.  The kernel also zeroes the top-k workspace the NEXT round will use.
// The sharded round (sdpcut_shard_finish_round) uses it with d_c4 == NULL (all cap entries exist,
// those of other shards get ks = 0 / lam = NaN) and a header of world x 64 bytes written elsewhere.
__global__ __launch_bounds__(64) void round_rows_kernel(int64_t cap, const int64_t *d_c4, const int64_t *idx,
                                                        const double *score, int64_t idx_base, int64_t n_local,
                                                        const int32_t *set5, const int32_t *ks, const double *vars,
                                                        int32_t nv, int64_t L, int coef_ld, char *block,
                                                        int64_t hdr_bytes, uint64_t *zero_ptr, int zero_words,
                                                        int64_t done_serial, uint32_t *done_ticket, const double *eig)
{
    __shared__ double tile[64 * SDPCUT_ROW_LD];
    const int lane = threadIdx.x;
    for (int w = blockIdx.x * 64 + lane; w < zero_words; w += gridDim.x * 64) zero_ptr[w] = 0ull;
    int64_t *o_c4 = (int64_t *)block;
    int64_t *o_idx = (int64_t *)(block + hdr_bytes);
    double *o_score = (double *)(o_idx + cap);
    double *o_lam = o_score + cap;
    double *o_rhs = o_lam + cap;
    double *o_coef = o_rhs + cap;
    int32_t *o_ks = (int32_t *)(o_coef + cap * coef_ld);
    const int64_t first = (int64_t)blockIdx.x * 64;
    const int64_t i = first + lane;
    // (requested before the head's length is known: one dependent trip to memory less on the critical path of a
    // kernel that is a chain of them; an entry beyond the head is never dereferenced)
    const int64_t gid_any = i < cap ? idx[i] : 0;
    const double score_any = i < cap ? score[i] : 0.0;
    int64_t limit = cap;
    if (d_c4) {
        if (blockIdx.x == 0 && lane < 7) o_c4[lane] = d_c4[lane];     // counters, strong count, mode (TopkWs::counters)
        limit = d_c4[3];
        if (limit > cap) limit = cap;
    }
    if (i < limit) {
        const int64_t gid = gid_any;
        const int64_t c = gid - idx_base;
        double co[SDPCUT_ROW_LD];
        int64_t cl[SDPCUT_ROW_LD];
#pragma unroll
        for (int m = 0; m < SDPCUT_ROW_LD; ++m) co[m] = 0.0;
        double lam = __builtin_nan(""), rhs = 0.0;
        int k = 0;
        // ids and scores go out first: the kernel ends in a burst of 0.54 MB over PCIe (~8 us at the link's rate, most of
        // what the kernel takes beyond its launch) -- what is known before the eigenvectors travels while they are computed
        o_idx[i] = gid;
        o_score[i] = score_any;
        if (c >= 0 && c < n_local) {
            k = ks[c];
            const int32_t *s5 = set5 + c * 5;
            CALL_FOR_SET_SIZE(k, cut_row_one, s5, vars, nv, L, &lam, co, &rhs, cl, eig ? eig + c : nullptr);
        }
        o_lam[i] = lam;
        o_rhs[i] = rhs;
        o_ks[i] = k;
#pragma unroll
        for (int m = 0; m < SDPCUT_ROW_LD; ++m)
            if (m < coef_ld) tile[lane * coef_ld + m] = co[m];
    }
    wave_lds_sync();
    const int64_t nlive = (limit - first < 64) ? limit - first : 64;
    const int total = nlive > 0 ? (int)nlive * coef_ld : 0;
    for (int w = lane; w < total; w += 64) o_coef[first * coef_ld + w] = tile[w];
    if (done_serial) publish_round_done(done_ticket, o_c4 + 7, done_serial);
}

// ------------------------------------------------------------------------------------------
// Epilogue of a fused round in CSR form (sdpcut_round_csr): what _gen_eigcuts_selected appends to the LP,
// cut_select_qp.py:737-754 -- for the ranked head: eigh, skip unless lambda_min < -1e-15, zero the tiny
// components, coefficients on the columns [L + i for i in set_inds] + Xarr_inds, rhs -v0^2 -- as ONE block
// of rows in compressed sparse row form, assembled on the device and stored straight into the pinned host
// block.  The host-side assembly of the padded rows (boolean masks over [5000, 20] arrays, column indices
// from the index sets) cost 1-3 ms per round, more than the whole device side of the round.
//
// One lane per head entry, 64 entries per workgroup.  A cut's position in the block (row number, offset of
// its non-zeros) is the number of cuts / non-zeros in front of it in head order: inside the workgroup a
// wave scan, across workgroups the look-back of rows_dev.h (csr_lookback).
struct RoundCsrArgs {
    int64_t cap;               // head entries the block is laid out for
    const int64_t *d_c4;       // TopkWs::counters of the selection (k_eff at [3]); NULL: `limit` entries exist
    int64_t limit;
    const int64_t *idx;        // [cap] global candidate ids of the head
    const double *score;       // [cap]
    int64_t idx_base, n_local;
    const int32_t *set5;       // [N][5] index sets in caller order
    const int32_t *ks;         // [N]
    const double *vars;
    int32_t nv;
    int64_t L;
    const double *eig;         // [N] lambda_min of every candidate at this point if the scoring pass computed it, else NULL
    // outputs: device view of the pinned host block
    int64_t *o_hdr;            // [16]: 0..6 selection counters, 7 completion serial, 8 cuts, 9 non-zeros, 10 look-back gave up
                               // (the host zeroes word 10 before the launch)
    int64_t *o_idx;            // [cap]
    double *o_score;           // [cap]
    double *o_lam;             // [cap]
    int32_t *o_ks;             // [cap]
    int32_t *o_sets;           // [cap][5]
    int32_t *o_row_entry;      // [cap]    head position of cut r
    int32_t *o_indptr;         // [cap + 1]
    double *o_rhs;             // [cap]
    int32_t *o_indices;        // [cap * ld]
    double *o_values;          // [cap * ld]
    uint64_t *zero_ptr;        // top-k workspace of the next round (zeroed here, see round_rows_kernel)
    int zero_words;
    int64_t serial;
    uint32_t *done_ticket;
    uint64_t *agg;             // [gridDim.x] look-back words
    int inject;                // SDPCUT_OPT_INJECT_GIVEUP: the look-back gives up unasked (rows_dev.h); 0 outside tests
};

#ifndef ROUND_MIN_BLOCKS
#define ROUND_MIN_BLOCKS 8      // workgroups of an epilogue launch at least (they share the zeroing of the next round's top-k workspace)
#endif

// The assembly itself: workgroup blockIdx.x of the gridDim.x that serve ONE head (round_csr_kernel: the launch; the batched
// kernel below: one row of its grid).  Everything but the zeroing of the next round's workspace and the completion word.
__device__ __forceinline__ void round_csr_body(const RoundCsrArgs &R)
{
    __shared__ double s_val[64 * SDPCUT_ROW_LD];
    __shared__ int32_t s_ind[64 * SDPCUT_ROW_LD];
    const int lane = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * 64;
    const int64_t i = first + lane;
    const int64_t gid_any = i < R.cap ? R.idx[i] : 0;
    const double score_any = i < R.cap ? R.score[i] : 0.0;
    int64_t limit = R.limit;
    if (R.d_c4) {
        if (blockIdx.x == 0 && lane < 7) R.o_hdr[lane] = R.d_c4[lane];
        limit = R.d_c4[3];
    }
    if (limit > R.cap) limit = R.cap;
    double co[SDPCUT_ROW_LD];
    int64_t cl[SDPCUT_ROW_LD];
#pragma unroll
    for (int m = 0; m < SDPCUT_ROW_LD; ++m) { co[m] = 0.0; cl[m] = 0; }
    double lam = __builtin_nan(""), rhs = 0.0;
    int k = 0;
    if (i < limit) {
        R.o_idx[i] = gid_any;
        R.o_score[i] = score_any;
        const int64_t c = gid_any - R.idx_base;
        int32_t s5[5] = {-1, -1, -1, -1, -1};
        if (c >= 0 && c < R.n_local) {
            k = R.ks[c];
            const int32_t *sp = R.set5 + c * 5;
#pragma unroll
            for (int a = 0; a < 5; ++a) s5[a] = sp[a];
            CALL_FOR_SET_SIZE(k, cut_row_one, sp, R.vars, R.nv, R.L, &lam, co, &rhs, cl, R.eig ? R.eig + c : nullptr);
        }
        R.o_lam[i] = lam;
        R.o_ks[i] = k;
#pragma unroll
        for (int a = 0; a < 5; ++a) R.o_sets[i * 5 + a] = s5[a];
    }
    const bool keep = i < limit && k > 0 && lam < SDPCUT_NEG_EIGVAL;       // :739
    const int len = keep ? k * (k + 3) / 2 : 0;
    // position inside the workgroup (= one wave)
    const unsigned long long km = __ballot(keep);
    const int my_row = __popcll(km & ((1ull << lane) - 1ull));
    const int wg_rows = __popcll(km);
    int incl = len;
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    const int my_off = incl - len;
    const int wg_nnz = __shfl(incl, 63);
    // publish this workgroup's aggregate, then sum those of the workgroups in front
    int64_t pre_rows, pre_nnz;
    const int gave_up = csr_lookback(R.agg, (uint32_t)R.serial, wg_rows, wg_nnz, pre_rows, pre_nnz, R.inject);
    if (gave_up && lane == 0) R.o_hdr[10] = 1;      // the block is void; the host launches the assembly once more (round.hip: csr_assemble_wait)
    if (keep) {
        const int64_t r = pre_rows + my_row;
        R.o_row_entry[r] = (int32_t)i;
        R.o_indptr[r] = (int32_t)(pre_nnz + my_off);
        R.o_rhs[r] = rhs;
#pragma unroll
        for (int m = 0; m < SDPCUT_ROW_LD; ++m)
            if (m < len) { s_val[my_off + m] = co[m]; s_ind[my_off + m] = (int32_t)cl[m]; }
    }
    wave_lds_sync();
    for (int w = lane; w < wg_nnz; w += 64) {      // contiguous, coalesced stores over PCIe
        R.o_values[pre_nnz + w] = s_val[w];
        R.o_indices[pre_nnz + w] = s_ind[w];
    }
    if (blockIdx.x == gridDim.x - 1 && lane == 0) {
        R.o_indptr[pre_rows + wg_rows] = (int32_t)(pre_nnz + wg_nnz);
        R.o_hdr[8] = pre_rows + wg_rows;
        R.o_hdr[9] = pre_nnz + wg_nnz;
    }
}

__global__ __launch_bounds__(64) void round_csr_kernel(RoundCsrArgs R)
{
    const int lane = threadIdx.x;
    for (int w = blockIdx.x * 64 + lane; w < R.zero_words; w += gridDim.x * 64) R.zero_ptr[w] = 0ull;
    round_csr_body(R);
    publish_round_done(R.done_ticket, R.o_hdr + 7, R.serial);
}

// The same assembly for the P points of a batch (sdpcut_round_csr_points, points.hip): row y of the grid serves point p_first + y --
// its own head (ids, scores, selection counters), LP point and lambda_min array, its own slice of the pinned batch block (header
// with counters, n_rows, nnz and the give-up flag included) and its own look-back words, so a workgroup still only waits for
// workgroups in front of it in its own row.  R describes point 0; the strides are applied to the kernel argument before the
// unchanged body runs.  No workspace to zero and no completion word: the host waits for the stream.
struct RoundCsrPointStrides {
    int32_t p_first;
    int64_t c4;        // int64 words between the selection counters of two points (sizeof(TopkWs) / 8)
    int64_t head;      // entries between two heads (cap)
    int64_t vars;      // doubles between two LP points
    int64_t eig;       // doubles between two lambda_min arrays
    int64_t block;     // BYTES between two slices of the batch block
    int64_t agg;       // look-back words per point
};

template <class T> __device__ __forceinline__ void shift_bytes(T *&p, int64_t off) { p = (T *)((char *)p + off); }

__global__ __launch_bounds__(64) void round_csr_points_kernel(RoundCsrArgs R, RoundCsrPointStrides ps)
{
    const int64_t p = (int64_t)ps.p_first + (int64_t)blockIdx.y;
    R.d_c4 += p * ps.c4;
    R.idx += p * ps.head;
    R.score += p * ps.head;
    R.vars += p * ps.vars;
    if (R.eig) R.eig += p * ps.eig;
    const int64_t off = p * ps.block;
    shift_bytes(R.o_hdr, off); shift_bytes(R.o_idx, off); shift_bytes(R.o_score, off); shift_bytes(R.o_lam, off);
    shift_bytes(R.o_ks, off); shift_bytes(R.o_sets, off); shift_bytes(R.o_row_entry, off); shift_bytes(R.o_indptr, off);
    shift_bytes(R.o_rhs, off); shift_bytes(R.o_indices, off); shift_bytes(R.o_values, off);
    R.agg += p * ps.agg;
    round_csr_body(R);
}

// LP point: mapped host memory -> device table (sdpcut_set_point)
__global__ __launch_bounds__(256) void point_copy_kernel(const double *src, double *dst, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = src[i];
}

// ------------------------------------------------------------------------------------------
// host launchers

// The completion ticket and the look-back words of the handle's row assemblies (common.h: ROUND_TICKET_BYTES, ROUND_AGG_WORDS),
// allocated by the first launch that needs them; zero once: the ticket returns to zero with every launch, and no look-back word
// carries a serial yet (serials start at 1).  The plain, the diverse and the multi-cut round share them: no two assemblies of one
// handle run at the same time, because every route refuses to start while a round is pending (SDPCUT_NO_PENDING) and waits for
// its own assembly before it returns.
int ensure_round_sync(sdpcut_ctx *h)
{
    if (h->d_done_ticket.get()) return 0;
    const size_t bytes = ROUND_TICKET_BYTES + (size_t)ROUND_AGG_WORDS * 8;
    HIP_TRY(h, h->d_done_ticket.reset(bytes / sizeof(uint32_t)));
    HIP_TRY(h, hipMemsetAsync(h->d_done_ticket.get(), 0, bytes, h->stream));
    return 0;
}

// output pointers of a CSR assembly into the block (device view) of a head of cap entries with rows of ld (round_layout.h: csr_layout)
static void csr_args_out(RoundCsrArgs &R, void *block, int64_t cap, int ld)
{
    const CsrLayout y = csr_layout(cap, ld);
    char *b = (char *)block;
    R.o_hdr = (int64_t *)b;
    R.o_idx = (int64_t *)(b + y.idx); R.o_score = (double *)(b + y.score); R.o_lam = (double *)(b + y.lam);
    R.o_rhs = (double *)(b + y.rhs); R.o_values = (double *)(b + y.values); R.o_ks = (int32_t *)(b + y.ks);
    R.o_sets = (int32_t *)(b + y.sets); R.o_row_entry = (int32_t *)(b + y.row_entry); R.o_indptr = (int32_t *)(b + y.indptr);
    R.o_indices = (int32_t *)(b + y.indices);
}
int launch_cut_rows(sdpcut_ctx *h, int64_t count, const int64_t *d_limit, const int64_t *d_idx, int64_t idx_base,
                    double *d_lam, double *d_coef, int coef_ld, double *d_rhs, int64_t *d_cols, int32_t *d_ks)
{
    if (count == 0) return 0;
    const int grid = (int)((count + 63) / 64);
    hipLaunchKernelGGL(cut_rows_kernel, dim3(grid), dim3(64), 0, h->stream, count, d_limit, d_idx, idx_base,
                       h->N, h->d_set_orig.get(), h->d_k.get(), h->d_vars.get(), h->nb_vars, h->L, d_lam, d_coef, coef_ld, d_rhs, d_cols,
                       d_ks, (h->scored & SDPCUT_EIG) ? (const double *)h->d_eig.get() : (const double *)nullptr);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

int launch_point_copy(sdpcut_ctx *h, const double *src_mapped, int64_t n)
{
    int64_t g = (n + 255) / 256;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(point_copy_kernel, dim3((unsigned)(g < 1 ? 1 : g)), dim3(256), 0, h->stream, src_mapped, h->d_vars.get(), n);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

int launch_round_rows(sdpcut_ctx *h, int64_t cap, const int64_t *d_c4, const int64_t *d_idx, const double *d_score,
                      int coef_ld, void *block, int64_t hdr_bytes, int64_t done_serial)
{
    if (cap <= 0) return 0;
    int rc;
    if (done_serial && (rc = ensure_round_sync(h))) return rc;
    uint64_t *zp = nullptr;
    int zw = 0;
    rc = topk_alt_ws(h, &zp, &zw);
    if (rc) return rc;
    int grid = (int)((cap + 63) / 64);
    if (grid < ROUND_MIN_BLOCKS) grid = ROUND_MIN_BLOCKS;      // (the workspace zeroing, see launch_round_csr)
    hipLaunchKernelGGL(round_rows_kernel, dim3(grid), dim3(64), 0, h->stream, cap, d_c4, d_idx, d_score, h->base, h->N,
                       h->d_set_orig.get(), h->d_k.get(), h->d_vars.get(), h->nb_vars, h->L, coef_ld, (char *)block, hdr_bytes, zp, zw, done_serial,
                       h->d_done_ticket.get(), (h->scored & SDPCUT_EIG) ? (const double *)h->d_eig.get() : (const double *)nullptr);
    HIP_TRY(h, hipGetLastError());
    h->topk_alt_clean = true;
    return 0;
}


int launch_round_csr(sdpcut_ctx *h, int64_t cap, const int64_t *d_c4, int64_t limit, const int64_t *d_idx, const double *d_score,
                     int ld, void *block, int64_t serial)
{
    if (cap <= 0) return 0;
    int grid = (int)((cap + 63) / 64);
    static_assert(256 <= ROUND_AGG_WORDS, "a look-back word per workgroup");
    if (grid > 256) return sdpcut_fail(h, SDPCUT_EINVAL, "round_csr: head too long");
    // (r4) the kernel also zeroes the next round's top-k workspace (124 KB): a head of a few entries is ONE workgroup, whose 64 lanes
    // then spend ~20 us on 242 stores each -- most of the epilogue of a QCQP round with 7 cuts.  Workgroups beyond the head only zero.
    if (grid < ROUND_MIN_BLOCKS) grid = ROUND_MIN_BLOCKS;
    int rc = ensure_round_sync(h);
    if (rc) return rc;
    RoundCsrArgs R;
    R.cap = cap; R.d_c4 = d_c4; R.limit = limit; R.idx = d_idx; R.score = d_score; R.idx_base = h->base; R.n_local = h->N;
    R.set5 = h->d_set_orig.get(); R.ks = h->d_k.get(); R.vars = h->d_vars.get(); R.nv = h->nb_vars; R.L = h->L;
    R.eig = (h->scored & SDPCUT_EIG) ? h->d_eig.get() : nullptr;
    csr_args_out(R, block, cap, ld);
    rc = topk_alt_ws(h, &R.zero_ptr, &R.zero_words);
    if (rc) return rc;
    R.serial = serial; R.done_ticket = h->d_done_ticket.get(); R.agg = round_agg_words(h);
    R.inject = inject_take(h, 2, cap > 64);
    hipLaunchKernelGGL(round_csr_kernel, dim3(grid), dim3(64), 0, h->stream, R);
    HIP_TRY(h, hipGetLastError());
    h->topk_alt_clean = true;
    return 0;
}

// CSR assembly of points [p_first, p_first + n_points) of a batch (round_csr_points_kernel).  Point p: head ids / scores at
// d_idx / d_score + p * cap, selection counters at d_c4 + p * c4_stride, LP point d_pts + p * pts_stride, lambda_min d_eig + p *
// eig_stride (d_eig NULL: the rows compute it), look-back words d_agg + p * agg_stride, slice block + p * block_stride.
int launch_round_csr_points(sdpcut_ctx *h, int p_first, int n_points, int64_t cap, int ld, const int64_t *d_c4, int64_t c4_stride,
                            const int64_t *d_idx, const double *d_score, const double *d_pts, int64_t pts_stride, const double *d_eig,
                            int64_t eig_stride, uint64_t *d_agg, int64_t agg_stride, void *block, int64_t block_stride, int64_t serial)
{
    if (cap <= 0 || n_points <= 0) return 0;
    const int grid = (int)((cap + 63) / 64);
    if (grid > agg_stride) return sdpcut_fail(h, SDPCUT_EINVAL, "round_csr_points: head too long");
    RoundCsrArgs R;
    R.cap = cap; R.d_c4 = d_c4; R.limit = cap; R.idx = d_idx; R.score = d_score; R.idx_base = h->base; R.n_local = h->N;
    R.set5 = h->d_set_orig.get(); R.ks = h->d_k.get(); R.vars = d_pts; R.nv = h->nb_vars; R.L = h->L;
    R.eig = d_eig;
    csr_args_out(R, block, cap, ld);
    R.zero_ptr = nullptr; R.zero_words = 0;
    R.serial = serial; R.done_ticket = nullptr; R.agg = d_agg;
    R.inject = inject_take(h, 2, cap > 64);
    RoundCsrPointStrides ps;
    ps.p_first = p_first; ps.c4 = c4_stride; ps.head = cap; ps.vars = pts_stride; ps.eig = eig_stride; ps.block = block_stride;
    ps.agg = agg_stride;
    hipLaunchKernelGGL(round_csr_points_kernel, dim3(grid, n_points), dim3(64), 0, h->stream, R, ps);
    HIP_TRY(h, hipGetLastError());
    return 0;
}
