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
// A boxed batch (sdpcut_score_points_boxed, sdpcut_round_csr_points_boxed) gives every point the variable bounds of its node.  Its
// (l | d) rows travel behind the points in the staging block and reach the device by an added row of points_copy_kernel; then
//   box_points_kernel         (box.hip) Q'_p and the transformed point p of every point, grid row = point
//   eig launch                on the ORIGINAL points: lambda_min knows no box
//   score_mfma_points_kernel  flags = SDPCUT_NN on the transformed points, Q stride L: the measure of every node's small SDP
//   strong_points_kernel      combined strategy: neither launch saw both measures, so the strong class is counted here
// and the selection and the assembly run as they are -- they read scores, heads and the original points, never Q.  The split is
// the one launch_score makes for a single point with a box (score.hip); still ONE host wait.
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
// the one-workgroup selection.  A boxed batch launches one row more: row n_points copies the box_n doubles of the (l | d) table.
__global__ __launch_bounds__(256) void points_copy_kernel(const double *src, double *dst, int64_t n, TopkWs *ws, int n_points, const double *box_src,
                                                          double *box_dst, int64_t box_n)
{
    if ((int)blockIdx.y == n_points) {      // (uniform)
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < box_n; i += (int64_t)gridDim.x * 256) box_dst[i] = box_src[i];
        return;
    }
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

// The strong class of the combined strategy in a boxed batch: candidates of point p = blockIdx.y with obj > 0 and eig <
// SDPCUT_NEG_EIGVAL (the test of the score kernels, which count it themselves where one launch computes both measures), over row p
// of the batch's score arrays.  A ballot and a popcount per wave, one no-return atomic per workgroup into one of the replicas of
// ws[p].strong_rep; runs behind points_copy_kernel's reset in stream order.
__global__ __launch_bounds__(256) void strong_points_kernel(const double *eig, const double *obj, int64_t N, int64_t score_stride, TopkWs *ws)
{
    __shared__ uint32_t s_cnt;
    const int64_t p = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const bool strong = i < N && obj[p * score_stride + i] > 0.0 && eig[p * score_stride + i] < SDPCUT_NEG_EIGVAL;
    const unsigned long long m = __ballot(strong);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&s_cnt, (uint32_t)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt)
        __hip_atomic_fetch_add((unsigned long long *)&ws[p].strong_rep[blockIdx.x % TK_SREP], (unsigned long long)s_cnt, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
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
    (void)hipFree(b.d_box_ld); (void)hipFree(b.d_Q_box); (void)hipFree(b.d_vars_box);
    b = PointsBufs();
}

// staging (pinned, mapped) and device table for P points; boxed: the staging block also holds the [P][2 n] (l | d) rows behind the
// points, and the device has a table for them
static int ensure_points_table(sdpcut_ctx *h, int P, bool boxed)
{
    PointsBufs &b = h->pts;
    const size_t doubles = (size_t)P * (size_t)(h->L + h->nb_vars);
    const size_t box_doubles = boxed ? (size_t)P * 2 * (size_t)h->nb_vars : 0;
    if (b.stage_bytes < (doubles + box_doubles) * 8) {
        HIP_TRY(h, sdpcut_sync(h));
        if (b.stage) (void)hipHostFree(b.stage);
        b.stage = b.stage_dev = nullptr;
        b.stage_bytes = 0;
        HIP_TRY(h, hipHostMalloc(&b.stage, (doubles + box_doubles) * 8, hipHostMallocMapped));
        HIP_TRY(h, hipHostGetDevicePointer(&b.stage_dev, b.stage, 0));
        b.stage_bytes = (doubles + box_doubles) * 8;
    }
    if (b.box_ld_doubles < box_doubles) {
        (void)hipFree(b.d_box_ld);
        b.d_box_ld = nullptr;
        b.box_ld_doubles = 0;
        HIP_TRY(h, hipMalloc((void **)&b.d_box_ld, box_doubles * 8));
        b.box_ld_doubles = box_doubles;
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

// Q' and the transformed points of a boxed batch of P points (batch_route.h: batch_box_table_bytes)
static int ensure_box_tables(sdpcut_ctx *h, int P)
{
    PointsBufs &b = h->pts;
    const size_t q = (size_t)P * (size_t)h->L, v = (size_t)P * (size_t)(h->L + h->nb_vars);
    if (b.box_q_doubles >= q && b.box_vars_doubles >= v) return 0;
    (void)hipFree(b.d_Q_box); (void)hipFree(b.d_vars_box);
    b.d_Q_box = b.d_vars_box = nullptr;
    b.box_q_doubles = b.box_vars_doubles = 0;
    HIP_TRY(h, hipMalloc((void **)&b.d_Q_box, q * 8));
    HIP_TRY(h, hipMalloc((void **)&b.d_vars_box, v * 8));
    b.box_q_doubles = q;
    b.box_vars_doubles = v;
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

// the boxes of a boxed batch as the caller hands them over: row p of lb / ub (stride ld) is the box of point p
struct BoxRows {
    const double *lb, *ub;
    int64_t ld;
};

// Both boxed calls leave the handle without a box, whichever way they return (the loop route and a redone point set one).
struct NoBoxAfter {
    sdpcut_ctx *h;
    explicit NoBoxAfter(sdpcut_ctx *ctx) : h(ctx) {}
    ~NoBoxAfter()
    {
        if (!h->box_set) return;
        (void)sdpcut_sync(h);      // (launches of the last point's scoring read the box tables)
        h->box_set = false;
        h->box_lb.clear(); h->box_ub.clear();
    }
};

// the P points into the staging block and, by one launch, into the device table; ws: see points_copy_kernel.  bx (a boxed batch):
// the (l | d) rows as sdpcut_set_box forms them, behind the points, and by an added row of the same launch into pts.d_box_ld.
static int upload_points(sdpcut_ctx *h, int P, const double *points, int64_t point_ld, TopkWs *ws, const BoxRows *bx = nullptr)
{
    int rc = ensure_points_table(h, P, bx != nullptr);
    if (rc) return rc;
    const int64_t n = h->L + h->nb_vars, nv = h->nb_vars;
    for (int p = 0; p < P; ++p) std::memcpy((double *)h->pts.stage + (size_t)p * n, points + (size_t)p * point_ld, (size_t)n * 8);
    const size_t box_off = (size_t)P * (size_t)n;
    if (bx) {
        double *ld = (double *)h->pts.stage + box_off;
        for (int p = 0; p < P; ++p) {
            const double *lb = bx->lb + (size_t)p * bx->ld, *ub = bx->ub + (size_t)p * bx->ld;
            for (int64_t i = 0; i < nv; ++i) { ld[(size_t)p * 2 * nv + i] = lb[i]; ld[(size_t)p * 2 * nv + nv + i] = ub[i] - lb[i]; }
        }
    }
    int64_t g = (n + 255) / 256;
    if (g > 64) g = 64;
    hipLaunchKernelGGL(points_copy_kernel, dim3((unsigned)g, (unsigned)(P + (bx ? 1 : 0))), dim3(256), 0, h->stream, (const double *)h->pts.stage_dev,
                       h->pts.d_pts, n, ws, P, bx ? (const double *)h->pts.stage_dev + box_off : nullptr, bx ? h->pts.d_box_ld : nullptr,
                       bx ? (int64_t)P * 2 * nv : 0);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// what a boxed call checks beside its sibling's arguments, before any state changes: the arrays, the option that has no boxes,
// every box by sdpcut_set_box's rule
static int check_box_rows(sdpcut_ctx *h, const char *what, int P, const BoxRows &bx)
{
    if (!bx.lb || !bx.ub) return sdpcut_fail(h, SDPCUT_EINVAL, std::string(what) + ": lb or ub is NULL");
    if (bx.ld < h->nb_vars) return sdpcut_fail(h, SDPCUT_EINVAL, std::string(what) + ": box_ld must be at least n");
    if (h->exact_head) return sdpcut_fail(h, SDPCUT_ESTATE, std::string(what) + ": SDPCUT_OPT_EXACT_HEAD is on (reference-exact heads have no node box)");
    for (int p = 0; p < P; ++p) {
        const int rc = box_check(h, what, p, bx.lb + (size_t)p * bx.ld, bx.ub + (size_t)p * bx.ld);
        if (rc) return rc;
    }
    return 0;
}

// do the point-axis kernels serve the scoring of a batch?  A boxed batch scores each measure in a launch of its own.
static bool batch_score_served(const sdpcut_ctx *h, uint32_t flags, bool boxed)
{
    if (!boxed) return score_points_served(h, flags);
    return (!(flags & SDPCUT_EIG) || score_points_served(h, SDPCUT_EIG)) && (!(flags & SDPCUT_NN) || score_points_served(h, SDPCUT_NN));
}

// The scores of an uploaded batch into pts.d_eig / pts.d_obj.  Unboxed: one scoring of `flags`.  Boxed: lambda_min from the original
// points, the measure from the box tables (written here) -- the split of launch_score (score.hip) -- and, where `strong` is set,
// the strong count of every point by a kernel of its own.
static int score_batch(sdpcut_ctx *h, uint32_t flags, int P, bool boxed, int64_t *strong, int64_t strong_stride)
{
    PointsBufs &b = h->pts;
    const int64_t n = h->L + h->nb_vars;
    int rc;
    if (!boxed || !(flags & SDPCUT_NN)) return launch_score_points(h, flags, P, b.d_pts, n, b.d_eig, b.d_obj, h->N, strong, strong_stride);
    if ((rc = ensure_box_tables(h, P))) return rc;
    if ((flags & SDPCUT_EIG) && (rc = launch_score_points(h, SDPCUT_EIG, P, b.d_pts, n, b.d_eig, b.d_obj, h->N, nullptr, 0))) return rc;
    if ((rc = launch_box_points(h, P, b.d_pts, n, b.d_box_ld, b.d_Q_box, b.d_vars_box))) return rc;
    if ((rc = launch_score_points(h, SDPCUT_NN, P, b.d_vars_box, n, b.d_eig, b.d_obj, h->N, nullptr, 0, b.d_Q_box, h->L))) return rc;
    if (strong) {
        hipLaunchKernelGGL(strong_points_kernel, dim3((unsigned)((h->N + 255) / 256), (unsigned)P), dim3(256), 0, h->stream, (const double *)b.d_eig,
                           (const double *)b.d_obj, h->N, h->N, (TopkWs *)b.d_ws);
        HIP_TRY(h, hipGetLastError());
    }
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

// sdpcut_score_points (bx == NULL) and sdpcut_score_points_boxed under the name `what`
static int score_points_impl(sdpcut_ctx *h, const char *what, int32_t n_points, const double *points, int64_t point_ld, const BoxRows *bx,
                             uint32_t flags, double *eig_out, double *obj_out)
{
    int rc = check_points_args(h, n_points, points, point_ld);
    if (rc) return rc;
    if (flags & SDPCUT_SDP) return sdpcut_fail(h, SDPCUT_EINVAL, std::string(what) + ": SDPCUT_SDP is not served over several points; flags = SDPCUT_EIG | SDPCUT_NN");
    if (flags & SDPCUT_EFF) return sdpcut_fail(h, SDPCUT_EINVAL, std::string(what) + ": SDPCUT_EFF is not served over several points; flags = SDPCUT_EIG | SDPCUT_NN");
    if (!(flags & (SDPCUT_EIG | SDPCUT_NN)) || (flags & ~(uint32_t)(SDPCUT_EIG | SDPCUT_NN)))
        return sdpcut_fail(h, SDPCUT_EINVAL, "flags must be a combination of SDPCUT_EIG and SDPCUT_NN");
    if (((flags & SDPCUT_EIG) && !eig_out) || ((flags & SDPCUT_NN) && !obj_out))
        return sdpcut_fail(h, SDPCUT_EINVAL, "the output array of a measure that is asked for is NULL");
    SDPCUT_NO_PENDING(h);
    SDPCUT_NO_BOX(h, what);      // (the boxed call brings its boxes; the handle's own would be lost)
    if (bx && (rc = check_box_rows(h, what, n_points, *bx))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    NoPointAfter leave(h);
    NoBoxAfter unboxed(h);
    const int P = n_points;
    const size_t N = (size_t)h->N;
    if (!(flags & SDPCUT_NN)) bx = nullptr;      // lambda_min knows no box
    if (!batch_score_served(h, flags, bx != nullptr)) {      // a kernel variant without a point axis: point by point
        for (int p = 0; p < P; ++p) {
            if (bx && (rc = sdpcut_set_box(h, bx->lb + (size_t)p * bx->ld, bx->ub + (size_t)p * bx->ld))) return rc;
            if ((rc = sdpcut_set_point(h, points + (size_t)p * point_ld))) return rc;
            if ((rc = sdpcut_score(h, flags))) return rc;
            if ((rc = sdpcut_get_scores(h, (flags & SDPCUT_EIG) ? eig_out + p * N : nullptr, (flags & SDPCUT_NN) ? obj_out + p * N : nullptr))) return rc;
        }
        return SDPCUT_OK;
    }
    if ((rc = ensure_points_scores(h, P))) return rc;
    if ((rc = upload_points(h, P, points, point_ld, nullptr, bx))) return rc;
    if ((rc = score_batch(h, flags, P, bx != nullptr, nullptr, 0))) return rc;
    if (flags & SDPCUT_EIG) HIP_TRY(h, hipMemcpyAsync(eig_out, h->pts.d_eig, (size_t)P * N * 8, hipMemcpyDeviceToHost, h->stream));
    if (flags & SDPCUT_NN) HIP_TRY(h, hipMemcpyAsync(obj_out, h->pts.d_obj, (size_t)P * N * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

// sdpcut_round_csr_points (bx == NULL) and sdpcut_round_csr_points_boxed under the name `what`
static int round_csr_points_impl(sdpcut_ctx *h, const char *what, int32_t n_points, const double *points, int64_t point_ld, const BoxRows *bx,
                                 int strat, int64_t sel_size, sdpcut_round_csr_t *out)
{
    if (!out) return sdpcut_fail(h, SDPCUT_EINVAL, "out is NULL");
    int rc = check_points_args(h, n_points, points, point_ld);
    if (rc) return rc;
    if (strat == SDPCUT_STRAT_EFF)
        return sdpcut_fail(h, SDPCUT_EINVAL, std::string(what) + ": strategy 6 (efficacy) is not served over several points; strategies 1, 2 and 4 are");
    if (!batch_mode(strat))
        return sdpcut_fail(h, SDPCUT_EINVAL, std::string(what) + " serves strategies 1 (feasibility), 2 (optimality) and 4 (combined)");
    if (sel_size < 0) return sdpcut_fail(h, SDPCUT_EINVAL, "sel_size is negative");
    SDPCUT_NO_PENDING(h);
    SDPCUT_NO_BOX(h, what);
    if (bx && (rc = check_box_rows(h, what, n_points, *bx))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    NoPointAfter leave(h);
    NoBoxAfter unboxed(h);
    const int P = n_points;
    std::memset(out, 0, (size_t)P * sizeof(*out));
    const int64_t cap = sel_size < h->N ? sel_size : h->N;
    const int ld = h->row_len_max;
    const uint32_t need = strat_need(strat);
    const bool shard = h->base != 0 || h->shard_rec != nullptr;
    int route = bx ? batch_route_boxed(h->N, cap, strat, h->exact_head, shard, h->nb_vars, P) : batch_route(h->N, cap, strat, h->exact_head, shard);
    // the boxes reach the device only where the measure is scored (lambda_min knows no box); the per-point rounds always get theirs
    const BoxRows *bx_dev = (need & SDPCUT_NN) ? bx : nullptr;
    // what the route function does not see: a kernel variant without a point axis, the combined regime resolved on the host
    // (SDPCUT_OPT_AUTO_REGIME off), event timing of the single-point launches
    if (route == BATCH_FAST && (!batch_score_served(h, need, bx_dev != nullptr) || (strat == SDPCUT_STRAT_COMB && !h->auto_regime) || h->timing))
        route = BATCH_LOOP;
    const BatchLayout y = batch_layout(cap, ld, P);
    if ((rc = ensure_points_block(h, y.bytes))) return rc;
    char *block = (char *)h->pts.pinned;
    // one point through the single-point round, in its box where the batch has boxes
    auto single = [&](int p) -> int {
        int rc1;
        if (bx && (rc1 = sdpcut_set_box(h, bx->lb + (size_t)p * bx->ld, bx->ub + (size_t)p * bx->ld))) return rc1;
        return point_through_round(h, points + (size_t)p * point_ld, strat, sel_size, block + batch_point_offset(y, p), out + p);
    };
    if (route == BATCH_LOOP) {
        for (int p = 0; p < P; ++p)
            if ((rc = single(p))) return rc;
        return SDPCUT_OK;
    }

    if ((rc = ensure_points_scores(h, P))) return rc;
    if ((rc = ensure_points_select(h, P, cap))) return rc;
    PointsBufs &b = h->pts;
    TopkWs *ws = (TopkWs *)b.d_ws;
    const int64_t ws_words = (int64_t)(sizeof(TopkWs) / 8), n = h->L + h->nb_vars;
    if ((rc = upload_points(h, P, points, point_ld, ws, bx_dev))) return rc;
    // the strong class of the combined strategy: counted by the score launch (a boxed batch: by strong_points_kernel behind its two
    // launches), point p into ws[p].strong_rep
    int64_t *strong = need == (SDPCUT_EIG | SDPCUT_NN) ? ws->strong_rep : nullptr;
    if ((rc = score_batch(h, need, P, bx_dev != nullptr, strong, ws_words))) return rc;
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
        if ((rc = single(p))) return rc;
    }
    return SDPCUT_OK;
}

extern "C" {

int sdpcut_score_points(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, uint32_t flags, double *eig_out,
                        double *obj_out)
{
    if (!h) return SDPCUT_EINVAL;
    return score_points_impl(h, "sdpcut_score_points", n_points, points, point_ld, nullptr, flags, eig_out, obj_out);
}

int sdpcut_round_csr_points(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, int strat, int64_t sel_size,
                            sdpcut_round_csr_t *out)
{
    if (!h) return SDPCUT_EINVAL;
    return round_csr_points_impl(h, "sdpcut_round_csr_points", n_points, points, point_ld, nullptr, strat, sel_size, out);
}

int sdpcut_score_points_boxed(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, const double *lb, const double *ub,
                              int64_t box_ld, uint32_t flags, double *eig_out, double *obj_out)
{
    if (!h) return SDPCUT_EINVAL;
    const BoxRows bx = {lb, ub, box_ld};
    return score_points_impl(h, "sdpcut_score_points_boxed", n_points, points, point_ld, &bx, flags, eig_out, obj_out);
}

int sdpcut_round_csr_points_boxed(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, const double *lb, const double *ub,
                                  int64_t box_ld, int strat, int64_t sel_size, sdpcut_round_csr_t *out)
{
    if (!h) return SDPCUT_EINVAL;
    const BoxRows bx = {lb, ub, box_ld};
    return round_csr_points_impl(h, "sdpcut_round_csr_points_boxed", n_points, points, point_ld, &bx, strat, sel_size, out);
}

} // extern "C"
