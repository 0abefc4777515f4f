// Batched rounds: many LP points against ONE candidate list per call (include/sdpcut.h: sdpcut_score_points,
// sdpcut_round_csr_points).  A round on a short list costs its launch chain and the host hand-off, not arithmetic; a caller
// that separates at the open nodes of a tree pays that once per point.  Here the same round has a point dimension:
//   points_copy_kernel        the P points, pinned staging -> device table [P][L + n]; also resets the selection state of every point
//   score_mfma_points_kernel  (score_mfma.hip) / eig_only_points_kernel (eig.hip): the unchanged scoring bodies, grid row = point
//   tk_points_kernel          one workgroup per point: the algorithm of tk_smallsel_kernel<true> (topk_small_dev.h) -- select,
//                             sort, emit the head -- with key buffers for TK_SMALLSORT_N candidates
//   round_csr_points_kernel   (rows.hip) the CSR assembly, grid row = point, every point into its slice of the batch block
// and ONE host wait.  Which batches go this way is decided in batch_route.h; all others -- and single points whose selection
// declared itself void -- run the single-point round (round.hip) once per point inside the call, so the call serves any list.
#include <cstring>
#include <vector>

#include "batch_route.h"
#include "common.h"
#include "topk_small_dev.h"

// look-back words of the row assembly per point: a head of at most TK_TILE entries is TK_TILE / 64 workgroups
#define BATCH_AGG_WORDS (TK_TILE / 64)

// ------------------------------------------------------------------------------------------
// kernels

// Row y: point y of the staging block (mapped host memory, rows of n doubles) -> row y of the device table.  ws != NULL (a round
// follows): workgroup 0 of every row also clears what the point's selection accumulates into or leaves from an earlier batch --
// the strong replicas the score launch adds to, the counters (void flag included) and n_sel.  Nothing else of a TopkWs is read by
// the one-workgroup selection.
__global__ __launch_bounds__(256) void points_copy_kernel(const double *src, double *dst, int64_t n, TopkWs *ws)
{
    const int64_t p = blockIdx.y;
    const double *s = src + p * n;
    double *d = dst + p * n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) d[i] = s[i];
    if (ws && blockIdx.x == 0) {
        TopkWs *w = ws + p;
        const int t = threadIdx.x;
        if (t < TK_SREP) w->strong_rep[t] = 0;
        else if (t < TK_SREP + 8) w->counters[t - TK_SREP] = 0;
        else if (t == TK_SREP + 8) w->n_sel = 0;
    }
}

// Workgroup p selects, sorts and emits the head of point p: scores in row p of eig / obj (a measure the mode does not read: NULL),
// state and counters in ws[p] (the strong count of the combined strategy is what the score launch left in ws[p].strong_rep), head
// in row p of idx_out / score_out (k entries per row).  LDS: keys of TK_SMALLSORT_N candidates (32 KB) + the sort's 2048 keys and
// indices (24 KB) + histogram and tables: 59 064 bytes, and the kernel is compiled for 8 waves per SIMD (64 registers, nothing
// spilled to scratch): TWO workgroups of sixteen waves fit a CU (tk_smallsel_kernel<true>: 125 112 bytes, one).
__global__ __launch_bounds__(TK_SMALLSEL_THREADS, 8) void tk_points_kernel(int mode, int64_t sel, int n, int k, const double *eig, const double *obj,
                                                                        int64_t score_stride, TopkWs *ws, double score_add, int64_t *idx_out,
                                                                        double *score_out)
{
    const int64_t p = blockIdx.x;
    smallsel_body<true, TK_SMALLSORT_N>(mode, sel, n, k, eig ? eig + p * score_stride : nullptr, obj ? obj + p * score_stride : nullptr, ws + p,
                                        nullptr, nullptr, 0, score_add, idx_out + p * k, score_out + p * k);
}

// ------------------------------------------------------------------------------------------
// buffers (grown on demand; both calls are synchronous, so nothing is in flight when one is replaced)

void free_points_ws(sdpcut_ctx *h)
{
    PointsBufs &b = h->pts;
    if (b.stage) (void)hipHostFree(b.stage);
    if (b.pinned) (void)hipHostFree(b.pinned);
    (void)hipFree(b.d_pts); (void)hipFree(b.d_eig); (void)hipFree(b.d_obj); (void)hipFree(b.d_ws); (void)hipFree(b.d_idx);
    (void)hipFree(b.d_score); (void)hipFree(b.d_agg);
    b = PointsBufs();
}

// staging (pinned, mapped) and device table for P points
static int ensure_points_table(sdpcut_ctx *h, int P)
{
    PointsBufs &b = h->pts;
    const size_t doubles = (size_t)P * (size_t)(h->L + h->nb_vars);
    if (b.stage_bytes < doubles * 8) {
        HIP_TRY(h, sdpcut_sync(h));
        if (b.stage) (void)hipHostFree(b.stage);
        b.stage = b.stage_dev = nullptr;
        b.stage_bytes = 0;
        HIP_TRY(h, hipHostMalloc(&b.stage, doubles * 8, hipHostMallocMapped));
        HIP_TRY(h, hipHostGetDevicePointer(&b.stage_dev, b.stage, 0));
        b.stage_bytes = doubles * 8;
    }
    if (b.pts_doubles < doubles) {
        (void)hipFree(b.d_pts);
        b.d_pts = nullptr;
        b.pts_doubles = 0;
        HIP_TRY(h, hipMalloc((void **)&b.d_pts, doubles * 8));
        b.pts_doubles = doubles;
    }
    return 0;
}

static int ensure_points_scores(sdpcut_ctx *h, int P)
{
    PointsBufs &b = h->pts;
    const size_t doubles = (size_t)P * (size_t)h->N;
    if (b.score_doubles >= doubles) return 0;
    (void)hipFree(b.d_eig); (void)hipFree(b.d_obj);
    b.d_eig = b.d_obj = nullptr;
    b.score_doubles = 0;
    HIP_TRY(h, hipMalloc((void **)&b.d_eig, doubles * 8));
    HIP_TRY(h, hipMalloc((void **)&b.d_obj, doubles * 8));
    b.score_doubles = doubles;
    return 0;
}

static int ensure_points_block(sdpcut_ctx *h, size_t bytes)
{
    PointsBufs &b = h->pts;
    if (b.pinned_bytes >= bytes) return 0;
    HIP_TRY(h, sdpcut_sync(h));
    if (b.pinned) (void)hipHostFree(b.pinned);
    b.pinned = b.pinned_dev = nullptr;
    b.pinned_bytes = 0;
    HIP_TRY(h, hipHostMalloc(&b.pinned, bytes, hipHostMallocMapped));
    HIP_TRY(h, hipHostGetDevicePointer(&b.pinned_dev, b.pinned, 0));
    b.pinned_bytes = bytes;
    return 0;
}

// per-point selection state, heads and look-back words of the one-launch route
static int ensure_points_select(sdpcut_ctx *h, int P, int64_t cap)
{
    PointsBufs &b = h->pts;
    if (b.ws_points < P) {
        (void)hipFree(b.d_ws);
        b.d_ws = nullptr;
        b.ws_points = 0;
        HIP_TRY(h, hipMalloc(&b.d_ws, (size_t)P * sizeof(TopkWs)));
        HIP_TRY(h, hipMemsetAsync(b.d_ws, 0, (size_t)P * sizeof(TopkWs), h->stream));
        b.ws_points = P;
    }
    const size_t entries = (size_t)P * (size_t)cap;
    if (b.head_entries < entries) {
        (void)hipFree(b.d_idx); (void)hipFree(b.d_score);
        b.d_idx = nullptr; b.d_score = nullptr;
        b.head_entries = 0;
        HIP_TRY(h, hipMalloc((void **)&b.d_idx, entries * 8));
        HIP_TRY(h, hipMalloc((void **)&b.d_score, entries * 8));
        // (a void selection emits no head, the assembly still reads its rows: never uninitialised memory)
        HIP_TRY(h, hipMemsetAsync(b.d_idx, 0, entries * 8, h->stream));
        HIP_TRY(h, hipMemsetAsync(b.d_score, 0, entries * 8, h->stream));
        b.head_entries = entries;
    }
    if (b.agg_points < P) {
        (void)hipFree(b.d_agg);
        b.d_agg = nullptr;
        b.agg_points = 0;
        HIP_TRY(h, hipMalloc((void **)&b.d_agg, (size_t)P * BATCH_AGG_WORDS * 8));
        HIP_TRY(h, hipMemsetAsync(b.d_agg, 0, (size_t)P * BATCH_AGG_WORDS * 8, h->stream));
        b.agg_points = P;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// host side

// the argument checks both calls share (the handle itself has been checked)
static int check_points_args(sdpcut_ctx *h, int32_t n_points, const double *points, int64_t point_ld)
{
    if (n_points < 1 || n_points > SDPCUT_BATCH_MAX_POINTS)
        return sdpcut_fail(h, SDPCUT_EINVAL, "n_points must be 1 .. SDPCUT_BATCH_MAX_POINTS (" + std::to_string(SDPCUT_BATCH_MAX_POINTS) + ")");
    if (!points) return sdpcut_fail(h, SDPCUT_EINVAL, "points is NULL");
    if (!h->d_vars) return sdpcut_fail(h, SDPCUT_ESTATE, "set_instance first");
    if (!h->d_eig || h->N < 1) return sdpcut_fail(h, SDPCUT_ESTATE, "set_candidates first");
    if (point_ld < h->L + h->nb_vars) return sdpcut_fail(h, SDPCUT_EINVAL, "point_ld must be at least L + n");
    return 0;
}

// Both calls leave the handle without a current point, whichever way they return: the single-point arrays hold, at best, the
// scores of the last point the per-point fallback served.
struct NoPointAfter {
    sdpcut_ctx *h;
    explicit NoPointAfter(sdpcut_ctx *ctx) : h(ctx) {}
    ~NoPointAfter()
    {
        h->have_point = false;
        h->scored = 0; h->obj_partial = false;
        h->last_total = -1;
    }
};

// the P points into the staging block and, by one launch, into the device table; ws: see points_copy_kernel
static int upload_points(sdpcut_ctx *h, int P, const double *points, int64_t point_ld, TopkWs *ws)
{
    int rc = ensure_points_table(h, P);
    if (rc) return rc;
    const int64_t n = h->L + h->nb_vars;
    for (int p = 0; p < P; ++p) std::memcpy((double *)h->pts.stage + (size_t)p * n, points + (size_t)p * point_ld, (size_t)n * 8);
    int64_t g = (n + 255) / 256;
    if (g > 64) g = 64;
    hipLaunchKernelGGL(points_copy_kernel, dim3((unsigned)g, (unsigned)P), dim3(256), 0, h->stream, (const double *)h->pts.stage_dev, h->pts.d_pts, n,
                       ws);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// One point through the single-point round (sdpcut_round_csr: the handle's single-point arrays and pinned block are its scratch);
// the block it returns is copied into `slot` and *out points there.
static int point_through_round(sdpcut_ctx *h, const double *point, int strat, int64_t sel_size, char *slot, sdpcut_round_csr_t *out)
{
    const int rc = sdpcut_round_csr(h, point, strat, sel_size, out);
    if (rc) return rc;
    if (out->cap > 0 && out->idx) {
        std::memcpy(slot, h->pinned, csr_layout(out->cap, out->row_ld).bytes);
        csr_out_from_block(slot, out);
    }
    return SDPCUT_OK;
}

extern "C" {

int sdpcut_score_points(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, uint32_t flags, double *eig_out,
                        double *obj_out)
{
    if (!h) return SDPCUT_EINVAL;
    int rc = check_points_args(h, n_points, points, point_ld);
    if (rc) return rc;
    if (flags & SDPCUT_SDP) return sdpcut_fail(h, SDPCUT_EINVAL, "sdpcut_score_points: SDPCUT_SDP is not served over several points; flags = SDPCUT_EIG | SDPCUT_NN");
    if (!(flags & (SDPCUT_EIG | SDPCUT_NN)) || (flags & ~(uint32_t)(SDPCUT_EIG | SDPCUT_NN)))
        return sdpcut_fail(h, SDPCUT_EINVAL, "flags must be a combination of SDPCUT_EIG and SDPCUT_NN");
    if (((flags & SDPCUT_EIG) && !eig_out) || ((flags & SDPCUT_NN) && !obj_out))
        return sdpcut_fail(h, SDPCUT_EINVAL, "the output array of a measure that is asked for is NULL");
    SDPCUT_NO_PENDING(h);
    SDPCUT_NO_BOX(h, "sdpcut_score_points");      // (one Q for all points; a per-point Q' stride is a later step)
    HIP_TRY(h, hipSetDevice(h->device));
    NoPointAfter leave(h);
    const int P = n_points;
    const size_t N = (size_t)h->N;
    if (!score_points_served(h, flags)) {      // a kernel variant without a point axis: point by point
        for (int p = 0; p < P; ++p) {
            if ((rc = sdpcut_set_point(h, points + (size_t)p * point_ld))) return rc;
            if ((rc = sdpcut_score(h, flags))) return rc;
            if ((rc = sdpcut_get_scores(h, (flags & SDPCUT_EIG) ? eig_out + p * N : nullptr, (flags & SDPCUT_NN) ? obj_out + p * N : nullptr))) return rc;
        }
        return SDPCUT_OK;
    }
    if ((rc = ensure_points_scores(h, P))) return rc;
    if ((rc = upload_points(h, P, points, point_ld, nullptr))) return rc;
    const int64_t n = h->L + h->nb_vars;
    rc = launch_score_points(h, flags, P, h->pts.d_pts, n, h->pts.d_eig, h->pts.d_obj, h->N, nullptr, 0);
    if (rc) return rc;
    if (flags & SDPCUT_EIG) HIP_TRY(h, hipMemcpyAsync(eig_out, h->pts.d_eig, (size_t)P * N * 8, hipMemcpyDeviceToHost, h->stream));
    if (flags & SDPCUT_NN) HIP_TRY(h, hipMemcpyAsync(obj_out, h->pts.d_obj, (size_t)P * N * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

int sdpcut_round_csr_points(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, int strat, int64_t sel_size,
                            sdpcut_round_csr_t *out)
{
    if (!h) return SDPCUT_EINVAL;
    if (!out) return sdpcut_fail(h, SDPCUT_EINVAL, "out is NULL");
    int rc = check_points_args(h, n_points, points, point_ld);
    if (rc) return rc;
    if (!batch_mode(strat))
        return sdpcut_fail(h, SDPCUT_EINVAL, "sdpcut_round_csr_points serves strategies 1 (feasibility), 2 (optimality) and 4 (combined)");
    if (sel_size < 0) return sdpcut_fail(h, SDPCUT_EINVAL, "sel_size is negative");
    SDPCUT_NO_PENDING(h);
    SDPCUT_NO_BOX(h, "sdpcut_round_csr_points");
    HIP_TRY(h, hipSetDevice(h->device));
    NoPointAfter leave(h);
    const int P = n_points;
    std::memset(out, 0, (size_t)P * sizeof(*out));
    const int64_t cap = sel_size < h->N ? sel_size : h->N;
    const int ld = h->row_len_max;
    const uint32_t need = strat_need(strat);
    int route = batch_route(h->N, cap, strat, h->exact_head, h->base != 0 || h->shard_rec != nullptr);
    // what the route function does not see: a kernel variant without a point axis, the combined regime resolved on the host
    // (SDPCUT_OPT_AUTO_REGIME off), event timing of the single-point launches
    if (route == BATCH_FAST && (!score_points_served(h, need) || (strat == SDPCUT_STRAT_COMB && !h->auto_regime) || h->timing)) route = BATCH_LOOP;
    const BatchLayout y = batch_layout(cap, ld, P);
    if ((rc = ensure_points_block(h, y.bytes))) return rc;
    char *block = (char *)h->pts.pinned;
    if (route == BATCH_LOOP) {
        for (int p = 0; p < P; ++p)
            if ((rc = point_through_round(h, points + (size_t)p * point_ld, strat, sel_size, block + batch_point_offset(y, p), out + p))) return rc;
        return SDPCUT_OK;
    }

    if ((rc = ensure_points_scores(h, P))) return rc;
    if ((rc = ensure_points_select(h, P, cap))) return rc;
    PointsBufs &b = h->pts;
    TopkWs *ws = (TopkWs *)b.d_ws;
    const int64_t ws_words = (int64_t)(sizeof(TopkWs) / 8), n = h->L + h->nb_vars;
    if ((rc = upload_points(h, P, points, point_ld, ws))) return rc;
    // the strong class of the combined strategy: counted by the score launch, point p into ws[p].strong_rep
    int64_t *strong = need == (SDPCUT_EIG | SDPCUT_NN) ? ws->strong_rep : nullptr;
    if ((rc = launch_score_points(h, need, P, b.d_pts, n, b.d_eig, b.d_obj, h->N, strong, ws_words))) return rc;
    const double *eig = (need & SDPCUT_EIG) ? b.d_eig : nullptr, *obj = (need & SDPCUT_NN) ? b.d_obj : nullptr;
    hipLaunchKernelGGL(tk_points_kernel, dim3((unsigned)P), dim3(TK_SMALLSEL_THREADS), 0, h->stream, batch_mode(strat), cap, (int)h->N, (int)cap, eig,
                       obj, h->N, ws, strat == SDPCUT_STRAT_COMB ? SDPCUT_BIG_M : 0.0, b.d_idx, b.d_score);
    HIP_TRY(h, hipGetLastError());
    for (int p = 0; p < P; ++p) std::memset(block + batch_point_offset(y, p), 0, 128);      // headers: counters, n_rows, nnz, give-up flag
    rc = launch_round_csr_points(h, 0, P, cap, ld, ws->counters, ws_words, b.d_idx, b.d_score, b.d_pts, n, eig, h->N, b.d_agg, BATCH_AGG_WORDS,
                                 b.pinned_dev, (int64_t)y.slice, ++h->round_serial);
    if (rc) return rc;
    HIP_TRY(h, sdpcut_sync(h));      // the one wait of the batch (a faulted kernel surfaces here as an error)

    std::vector<int> redo, again;
    for (int p = 0; p < P; ++p) {
        const int64_t *hdr = (const int64_t *)(block + batch_point_offset(y, p));
        sdpcut_round_csr_t &o = out[p];
        o.cap = cap;
        o.row_ld = ld;
        if (!rank_fast_finish(h, strat, sel_size, cap, hdr, &o.n_out, &o.n_total, &o.new_strat, o.counters)) {
            redo.push_back(p);      // a void selection: the single-point round resolves it (tie split or full sort)
            continue;
        }
        ++h->stat_rounds;
        if (hdr[10] && o.n_out > 0) again.push_back(p);
    }
    // a point whose row assembly gave up its bounded look-back (rows.hip): once more over the same head, like csr_assemble_wait (round.hip)
    for (int p : again) {
        int64_t *hdr = (int64_t *)(block + batch_point_offset(y, p));
        hdr[8] = hdr[9] = hdr[10] = 0;
        ++h->stat_fallbacks;
        rc = launch_round_csr_points(h, p, 1, cap, ld, ws->counters, ws_words, b.d_idx, b.d_score, b.d_pts, n, eig, h->N, b.d_agg, BATCH_AGG_WORDS,
                                     b.pinned_dev, (int64_t)y.slice, ++h->round_serial);
        if (rc) return rc;
    }
    if (!again.empty()) {
        HIP_TRY(h, sdpcut_sync(h));
        for (int p : again)
            if (((const int64_t *)(block + batch_point_offset(y, p)))[10])
                return sdpcut_fail(h, SDPCUT_EHIP, "round_csr_points: look-back of the row assembly timed out twice");
    }
    for (int p = 0; p < P; ++p) csr_out_from_block(block + batch_point_offset(y, p), out + p);      // (the redone ones are overwritten below)
    for (int p : redo) {
        ++h->stat_points_redone;
        std::memset(out + p, 0, sizeof(*out));
        if ((rc = point_through_round(h, points + (size_t)p * point_ld, strat, sel_size, block + batch_point_offset(y, p), out + p))) return rc;
    }
    return SDPCUT_OK;
}

} // extern "C"
