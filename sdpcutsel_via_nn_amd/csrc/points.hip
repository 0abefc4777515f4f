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
// The host side of a batched round is ONE driver, round_points, told by a PointsRound what differs between its callers:
//   intake and refusals, all before any state changes; the route (batch_route.h) and what overrides it; the batch block
//   BATCH_LOOP: every point through the single-point call, its block copied into the point's slice
//   BATCH_FAST: upload, scores, selection, row assembly, the one wait; then per point the verdict of its selection --
//     answered; answered, but the assembly gave up its bounded look-back: assembled once more, a second wait, an error if that
//     gives up too; void: redone through the single-point call, after everything else, over its slice
// The filtered batch (sdpcut_round_csr_points_diverse; strategies 1, 2, 4 and 6) is the same chain with a longer head and a filter
// (PointsFilter):
//   efficacy_points_kernel    (efficacy.hip) strategy 6: the efficacy score of every point, behind the eigenvalue launch
//   tk_points_kernel          k = the pool, the quota as `sel`
//   div_rows_points_kernel, div_points_kernel   (diverse.hip) the pool's rows, then one workgroup per point filters its pool in LDS
//   round_csr_points_kernel   over the accepted heads, their lengths read from the walk's counts
// its verdict reads the selection's counters where the filter left them, a ranking shorter than the quota gets the block of its
// own length, and the single-point call is sdpcut_round_csr_diverse.  sdpcut_efficacy_points is the eigenvalue launch and the
// efficacy launch alone.
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
// buffers (grown on demand through grow, common.h: the stream is waited for before a block is replaced)

// staging (pinned, mapped) and device table for P points; boxed: the staging block also holds the [P][2 n] (l | d) rows behind the
// points, and the device has a table for them
static int ensure_points_table(sdpcut_ctx *h, int P, bool boxed)
{
    PointsBufs &b = h->pts;
    const size_t doubles = (size_t)P * (size_t)(h->L + h->nb_vars);
    const size_t box_doubles = boxed ? (size_t)P * 2 * (size_t)h->nb_vars : 0;
    int rc;
    if ((rc = grow(h, b.stage, (doubles + box_doubles) * 8))) return rc;
    if ((rc = grow(h, b.d_box_ld, box_doubles))) return rc;
    return grow(h, b.d_pts, doubles);
}

static int ensure_points_scores(sdpcut_ctx *h, int P)
{
    PointsBufs &b = h->pts;
    const size_t doubles = (size_t)P * (size_t)h->N;
    const int rc = grow(h, b.d_eig, doubles);      // (the two are always asked for the same size: they grow together)
    return rc ? rc : grow(h, b.d_obj, doubles);
}

// Q' and the transformed points of a boxed batch of P points (batch_route.h: batch_box_table_bytes)
static int ensure_box_tables(sdpcut_ctx *h, int P)
{
    PointsBufs &b = h->pts;
    const size_t q = (size_t)P * (size_t)h->L, v = (size_t)P * (size_t)(h->L + h->nb_vars);
    const int rc = grow(h, b.d_Q_box, q);
    return rc ? rc : grow(h, b.d_vars_box, v);
}

// grow, and zero-fill what is new on the stream: the kernels that read these arrays rely on zeros where nothing was written yet
template <class T> static int grow_zeroed(sdpcut_ctx *h, DevBuf<T> &buf, size_t count)
{
    bool grew = false;
    const int rc = grow(h, buf, count, &grew);
    if (rc) return rc;
    if (grew) HIP_TRY(h, hipMemsetAsync(buf.get(), 0, count * sizeof(T), h->stream));
    return 0;
}

// per-point selection state, heads and look-back words of the one-launch route
static int ensure_points_select(sdpcut_ctx *h, int P, int64_t cap)
{
    PointsBufs &b = h->pts;
    const size_t entries = (size_t)P * (size_t)cap;
    int rc;
    if ((rc = grow_zeroed(h, b.d_ws, (size_t)P * sizeof(TopkWs)))) return rc;
    // (a void selection emits no head, the assembly still reads its rows: never uninitialised memory)
    if ((rc = grow_zeroed(h, b.d_idx, entries)) || (rc = grow_zeroed(h, b.d_score, entries))) return rc;
    return grow_zeroed(h, b.d_agg, (size_t)P * BATCH_AGG_WORDS);
}

// ------------------------------------------------------------------------------------------
// host side

// the shared intake checks and the state the batched rounds need (the handle itself has been checked)
static int check_batch_state(sdpcut_ctx *h, int32_t n_points, const double *points, int64_t point_ld)
{
    const int rc = check_point_batch(h, "", n_points, points, point_ld, h->L + h->nb_vars);
    if (rc) return rc;
    if (!h->d_vars.get()) return sdpcut_fail(h, SDPCUT_ESTATE, "set_instance first");
    if (!h->d_eig.get() || h->N < 1) return sdpcut_fail(h, SDPCUT_ESTATE, "set_candidates first");
    return 0;
}

// (NoPointAfter, NoBoxAfter -- what both calls leave the handle with -- are in common.h: the triangle batch shares them)

// the boxes of a boxed batch as the caller hands them over: row p of lb / ub (stride ld) is the box of point p
struct BoxRows {
    const double *lb, *ub;
    int64_t ld;
    const double *lo(int p) const { return lb + (size_t)p * ld; }      // the box of point p
    const double *hi(int p) const { return ub + (size_t)p * ld; }
};

// the P points into the staging block and, by one launch, into the device table; ws: see points_copy_kernel.  bx (a boxed batch):
// the (l | d) rows as sdpcut_set_box forms them, behind the points, and by an added row of the same launch into pts.d_box_ld.
static int upload_points(sdpcut_ctx *h, int P, const double *points, int64_t point_ld, TopkWs *ws, const BoxRows *bx = nullptr)
{
    int rc = ensure_points_table(h, P, bx != nullptr);
    if (rc) return rc;
    const int64_t n = h->L + h->nb_vars, nv = h->nb_vars;
    pack_points((double *)h->pts.stage.get(), P, points, point_ld, n);
    const size_t box_off = (size_t)P * (size_t)n;
    if (bx) pack_box_ld((double *)h->pts.stage.get() + box_off, P, nv, bx->lb, bx->ld, bx->ub, bx->ld);
    int64_t g = (n + 255) / 256;
    if (g > 64) g = 64;
    hipLaunchKernelGGL(points_copy_kernel, dim3((unsigned)g, (unsigned)(P + (bx ? 1 : 0))), dim3(256), 0, h->stream, (const double *)h->pts.stage.dev(),
                       h->pts.d_pts.get(), n, ws, P, bx ? (const double *)h->pts.stage.dev() + box_off : nullptr, bx ? h->pts.d_box_ld.get() : nullptr,
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
        const int rc = box_check(h, what, p, bx.lo(p), bx.hi(p));
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
    if (!boxed || !(flags & SDPCUT_NN)) return launch_score_points(h, flags, P, b.d_pts.get(), n, b.d_eig.get(), b.d_obj.get(), h->N, strong, strong_stride);
    if ((rc = ensure_box_tables(h, P))) return rc;
    if ((flags & SDPCUT_EIG) && (rc = launch_score_points(h, SDPCUT_EIG, P, b.d_pts.get(), n, b.d_eig.get(), b.d_obj.get(), h->N, nullptr, 0))) return rc;
    if ((rc = launch_box_points(h, P, b.d_pts.get(), n, b.d_box_ld.get(), b.d_Q_box.get(), b.d_vars_box.get()))) return rc;
    if ((rc = launch_score_points(h, SDPCUT_NN, P, b.d_vars_box.get(), n, b.d_eig.get(), b.d_obj.get(), h->N, nullptr, 0, b.d_Q_box.get(), h->L))) return rc;
    if (strong) {
        hipLaunchKernelGGL(strong_points_kernel, dim3((unsigned)((h->N + 255) / 256), (unsigned)P), dim3(256), 0, h->stream, (const double *)b.d_eig.get(),
                           (const double *)b.d_obj.get(), h->N, h->N, (TopkWs *)b.d_ws.get());
        HIP_TRY(h, hipGetLastError());
    }
    return 0;
}

// One point has gone through a single-point round (rc: what the call returned; the handle's single-point arrays and pinned block
// are its scratch): the block it returned is copied into `slot` and *out points there.
static int round_into_slot(sdpcut_ctx *h, int rc, char *slot, sdpcut_round_csr_t *out)
{
    if (rc) return rc;
    if (out->cap > 0 && out->idx) {
        std::memcpy(slot, h->pinned.get(), csr_layout(out->cap, out->row_ld).bytes);
        csr_out_from_block(slot, out);
    }
    return SDPCUT_OK;
}

// sdpcut_score_points (bx == NULL) and sdpcut_score_points_boxed under the name `what`
static int score_points_impl(sdpcut_ctx *h, const char *what, int32_t n_points, const double *points, int64_t point_ld, const BoxRows *bx,
                             uint32_t flags, double *eig_out, double *obj_out)
{
    int rc = check_batch_state(h, n_points, points, point_ld);
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
            if (bx && (rc = sdpcut_set_box(h, bx->lo(p), bx->hi(p)))) return rc;
            if ((rc = sdpcut_set_point(h, points + (size_t)p * point_ld))) return rc;
            if ((rc = sdpcut_score(h, flags))) return rc;
            if ((rc = sdpcut_get_scores(h, (flags & SDPCUT_EIG) ? eig_out + p * N : nullptr, (flags & SDPCUT_NN) ? obj_out + p * N : nullptr))) return rc;
        }
        return SDPCUT_OK;
    }
    if ((rc = ensure_points_scores(h, P))) return rc;
    if ((rc = upload_points(h, P, points, point_ld, nullptr, bx))) return rc;
    if ((rc = score_batch(h, flags, P, bx != nullptr, nullptr, 0))) return rc;
    if (flags & SDPCUT_EIG) HIP_TRY(h, hipMemcpyAsync(eig_out, h->pts.d_eig.get(), (size_t)P * N * 8, hipMemcpyDeviceToHost, h->stream));
    if (flags & SDPCUT_NN) HIP_TRY(h, hipMemcpyAsync(obj_out, h->pts.d_obj.get(), (size_t)P * N * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

// ------------------------------------------------------------------------------------------
// Efficacy and the filtered round over a batch (sdpcut_efficacy_points, sdpcut_round_csr_points_diverse)

static int ensure_points_eff(sdpcut_ctx *h, int P) { return grow(h, h->pts.d_eff, 3 * (size_t)P * (size_t)h->N); }

static_assert(DIVP_MAX_POOL == BATCH_DIVERSE_MAX_POOL && BATCH_DIVERSE_MAX_POOL <= TK_TILE, "the route's pool limit is the filter kernel's and fits a head of the selection");

// where the filter's arrays of a batch of P points lie inside pts.d_div
struct DivPointsLayout { size_t coef, lam, ks, info, acc_idx, acc_score, bytes; };
static DivPointsLayout div_points_layout(int P, int64_t pool, int64_t cap)
{
    DivPointsLayout y;
    const size_t e = (size_t)P * (size_t)pool, a = (size_t)P * (size_t)cap;
    size_t o = 0;
    y.coef = o; o += e * SDPCUT_ROW_LD * 8;
    y.lam = o; o += e * 8;
    y.ks = o; o += (e * 4 + 7) & ~(size_t)7;
    y.info = o; o += (size_t)P * 64;
    y.acc_idx = o; o += a * 8;
    y.acc_score = o; o += a * 8;
    y.bytes = o;
    return y;
}

static int ensure_points_div(sdpcut_ctx *h, int P, size_t bytes)
{
    // (the row assembly reads an accepted head up to its capacity and uses its length only: never uninitialised memory)
    const int rc = grow_zeroed(h, h->pts.d_div, bytes);
    return rc ? rc : grow(h, h->pts.div_sel, (size_t)P * 64);
}

// A block of csr_layout(from, ld) with n_out entries, n_rows rows and nnz non-zeros in use becomes one of csr_layout(to, ld), to <
// from, in place: every array moves towards the header, in the order they lie in.
static void csr_block_shrink(char *block, int64_t from, int64_t to, int ld, int64_t n_out, int64_t n_rows, int64_t nnz)
{
    const CsrLayout a = csr_layout(from, ld), z = csr_layout(to, ld);
    const size_t w = (size_t)n_out, r = (size_t)n_rows, nz = (size_t)nnz;
    std::memmove(block + z.idx, block + a.idx, w * 8);
    std::memmove(block + z.score, block + a.score, w * 8);
    std::memmove(block + z.lam, block + a.lam, w * 8);
    std::memmove(block + z.rhs, block + a.rhs, r * 8);
    std::memmove(block + z.values, block + a.values, nz * 8);
    std::memmove(block + z.ks, block + a.ks, w * 4);
    std::memmove(block + z.sets, block + a.sets, w * 20);
    std::memmove(block + z.row_entry, block + a.row_entry, r * 4);
    std::memmove(block + z.indptr, block + a.indptr, (r + 1) * 4);
    std::memmove(block + z.indices, block + a.indices, nz * 4);
}

static int efficacy_points_impl(sdpcut_ctx *h, int32_t n_points, const double *points, int64_t point_ld, double *eff_out, double *objpar_out,
                                double *escore_out)
{
    int rc = check_batch_state(h, n_points, points, point_ld);
    if (rc) return rc;
    if (!eff_out && !objpar_out && !escore_out) return sdpcut_fail(h, SDPCUT_EINVAL, "sdpcut_efficacy_points: every output array is NULL");
    SDPCUT_NO_PENDING(h);
    SDPCUT_NO_BOX(h, "sdpcut_efficacy_points");
    HIP_TRY(h, hipSetDevice(h->device));
    NoPointAfter leave(h);
    const int P = n_points;
    const size_t N = (size_t)h->N;
    if (!score_points_served(h, SDPCUT_EIG)) {      // a kernel variant without a point axis: point by point
        for (int p = 0; p < P; ++p) {
            if ((rc = sdpcut_set_point(h, points + (size_t)p * point_ld))) return rc;
            if ((rc = sdpcut_score(h, SDPCUT_EIG | SDPCUT_EFF))) return rc;
            if ((rc = sdpcut_get_efficacy(h, eff_out ? eff_out + p * N : nullptr, objpar_out ? objpar_out + p * N : nullptr,
                                          escore_out ? escore_out + p * N : nullptr)))
                return rc;
        }
        return SDPCUT_OK;
    }
    if ((rc = ensure_points_scores(h, P))) return rc;
    if ((rc = ensure_points_eff(h, P))) return rc;
    if ((rc = upload_points(h, P, points, point_ld, nullptr))) return rc;
    PointsBufs &b = h->pts;
    const int64_t n = h->L + h->nb_vars;
    if ((rc = score_batch(h, SDPCUT_EIG, P, false, nullptr, 0))) return rc;
    double *d_e = b.d_eff.get(), *d_p = d_e + (size_t)P * N, *d_s = d_p + (size_t)P * N;
    if ((rc = launch_efficacy_points(h, P, b.d_pts.get(), n, b.d_eig.get(), h->N, d_e, d_p, d_s))) return rc;
    if (eff_out) HIP_TRY(h, hipMemcpyAsync(eff_out, d_e, (size_t)P * N * 8, hipMemcpyDeviceToHost, h->stream));
    if (objpar_out) HIP_TRY(h, hipMemcpyAsync(objpar_out, d_p, (size_t)P * N * 8, hipMemcpyDeviceToHost, h->stream));
    if (escore_out) HIP_TRY(h, hipMemcpyAsync(escore_out, d_s, (size_t)P * N * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

// What the filtered batch adds to the plain one, and what differs between the two batched rounds: all the driver is told.
struct PointsFilter {
    int64_t pool_size;
    double max_parallel;
    sdpcut_diverse_info_t *info;      // [n_points] or NULL
};
struct PointsRound {
    const char *what;      // the entry point's name, for the refusals
    const BoxRows *bx;      // a box per point, or NULL
    int strat;
    int64_t sel_size;
    const PointsFilter *filter;      // NULL: sdpcut_round_csr_points[_boxed]
};

// The one-wait batched round: sdpcut_round_csr_points[_boxed] (R.filter == NULL) and sdpcut_round_csr_points_diverse.
static int round_points(sdpcut_ctx *h, const PointsRound &R, int32_t n_points, const double *points, int64_t point_ld, sdpcut_round_csr_t *out)
{
    const PointsFilter *F = R.filter;
    const BoxRows *bx = R.bx;
    const int strat = R.strat;
    const int64_t sel_size = R.sel_size;
    sdpcut_diverse_info_t *info = F ? F->info : nullptr;
    if (!out) return sdpcut_fail(h, SDPCUT_EINVAL, "out is NULL");
    int rc = check_batch_state(h, n_points, points, point_ld);
    if (rc) return rc;
    if (F) {
        if (!batch_mode_diverse(strat))
            return sdpcut_fail(h, SDPCUT_EINVAL, std::string(R.what) + " serves strategies 1 (feasibility), 2 (optimality), 4 (combined) and 6 (efficacy)");
        if (!(F->max_parallel >= 0.0 && F->max_parallel <= 1.0)) return sdpcut_fail(h, SDPCUT_EINVAL, "max_parallel must lie in [0, 1]");
        if (sel_size < 1) return sdpcut_fail(h, SDPCUT_EINVAL, "sel_size must be >= 1");
        if (F->pool_size < sel_size) return sdpcut_fail(h, SDPCUT_EINVAL, "pool_size must be >= sel_size");
        if (F->pool_size > SDPCUT_DIVERSE_MAX_POOL) return sdpcut_fail(h, SDPCUT_EINVAL, "pool_size must not exceed SDPCUT_DIVERSE_MAX_POOL");
    } else {
        if (strat == SDPCUT_STRAT_EFF)
            return sdpcut_fail(h, SDPCUT_EINVAL, std::string(R.what) + ": strategy 6 (efficacy) is not served over several points; strategies 1, 2 and 4 are");
        if (!batch_mode(strat))
            return sdpcut_fail(h, SDPCUT_EINVAL, std::string(R.what) + " serves strategies 1 (feasibility), 2 (optimality) and 4 (combined)");
        if (sel_size < 0) return sdpcut_fail(h, SDPCUT_EINVAL, "sel_size is negative");
    }
    SDPCUT_NO_PENDING(h);
    SDPCUT_NO_BOX(h, R.what);
    if (bx && (rc = check_box_rows(h, R.what, n_points, *bx))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    NoPointAfter leave(h);
    NoBoxAfter unboxed(h);
    const int P = n_points;
    std::memset(out, 0, (size_t)P * sizeof(*out));
    if (info) std::memset(info, 0, (size_t)P * sizeof(*info));
    const bool by_eff = strat == SDPCUT_STRAT_EFF;      // (the filtered batch only: strategy 2 on the efficacy score)
    // the quota, the head the selection emits (the filter's pool, else the quota) and the capacity of a slice of the batch block
    const int64_t sel = sel_size < h->N ? sel_size : h->N;
    const int64_t head = !F ? sel : F->pool_size < h->N ? F->pool_size : h->N;
    const int64_t cap = sel_size < head ? sel_size : head;
    const int ld = h->row_len_max;
    const uint32_t need = by_eff ? (uint32_t)SDPCUT_EIG : strat_need(strat);      // what score_batch computes; the efficacy launch follows it
    const bool shard = h->base != 0 || h->shard_rec != nullptr;
    int route;
    if (F)
        route = bx ? batch_route_diverse_boxed(h->N, sel_size, F->pool_size, strat, h->exact_head, shard, h->nb_vars, P)
                   : batch_route_diverse(h->N, sel_size, F->pool_size, strat, h->exact_head, shard);
    else
        route = bx ? batch_route_boxed(h->N, cap, strat, h->exact_head, shard, h->nb_vars, P) : batch_route(h->N, cap, strat, h->exact_head, shard);
    // the boxes reach the device only where the measure is scored (lambda_min knows no box); the per-point rounds always get theirs
    const BoxRows *bx_dev = (need & SDPCUT_NN) ? bx : nullptr;
    // what the route function does not see: a kernel variant without a point axis, the combined regime resolved on the host
    // (SDPCUT_OPT_AUTO_REGIME off), event timing of the single-point launches
    if (route == BATCH_FAST && (!batch_score_served(h, need, bx_dev != nullptr) || (strat == SDPCUT_STRAT_COMB && !h->auto_regime) || h->timing))
        route = BATCH_LOOP;
    const BatchLayout y = batch_layout(cap, ld, P);
    if ((rc = grow(h, h->pts.pinned, y.bytes))) return rc;
    char *block = (char *)h->pts.pinned.get();
    // one point through the single-point call (which also fills info[p]), in its box where the batch has boxes
    auto single = [&](int p) -> int {
        int rc1;
        if (bx && (rc1 = sdpcut_set_box(h, bx->lo(p), bx->hi(p)))) return rc1;
        const double *point = points + (size_t)p * point_ld;
        rc1 = F ? sdpcut_round_csr_diverse(h, point, strat, sel_size, F->pool_size, F->max_parallel, out + p, info ? info + p : nullptr)
                : sdpcut_round_csr(h, point, strat, sel_size, out + p);
        return round_into_slot(h, rc1, block + batch_point_offset(y, p), out + p);
    };
    if (route == BATCH_LOOP) {
        for (int p = 0; p < P; ++p)
            if ((rc = single(p))) return rc;
        return SDPCUT_OK;
    }

    if ((rc = ensure_points_scores(h, P))) return rc;
    if ((rc = ensure_points_select(h, P, head))) return rc;
    DivPointsLayout dy = {};
    if (F) {
        dy = div_points_layout(P, head, cap);
        if ((rc = ensure_points_div(h, P, dy.bytes))) return rc;
    }
    if (by_eff && (rc = ensure_points_eff(h, P))) return rc;
    PointsBufs &b = h->pts;
    TopkWs *ws = (TopkWs *)b.d_ws.get();
    const int64_t ws_words = (int64_t)(sizeof(TopkWs) / 8), n = h->L + h->nb_vars;
    if ((rc = upload_points(h, P, points, point_ld, ws, bx_dev))) return rc;
    // the strong class of the combined strategy: counted by the score launch (a boxed batch: by strong_points_kernel behind its two
    // launches), point p into ws[p].strong_rep
    int64_t *strong = need == (SDPCUT_EIG | SDPCUT_NN) ? ws->strong_rep : nullptr;
    if ((rc = score_batch(h, need, P, bx_dev != nullptr, strong, ws_words))) return rc;
    const double *eig = (need & SDPCUT_EIG) ? b.d_eig.get() : nullptr, *obj = (need & SDPCUT_NN) ? b.d_obj.get() : nullptr;
    if (by_eff) {      // strategy 2 on the efficacy score, as the single-point ranking runs it (common.h: MeasureAsObj)
        double *d_e = b.d_eff.get(), *d_p = d_e + (size_t)P * (size_t)h->N, *d_s = d_p + (size_t)P * (size_t)h->N;
        if ((rc = launch_efficacy_points(h, P, b.d_pts.get(), n, b.d_eig.get(), h->N, d_e, d_p, d_s))) return rc;
        obj = d_s;
    }
    hipLaunchKernelGGL(tk_points_kernel, dim3((unsigned)P), dim3(TK_SMALLSEL_THREADS), 0, h->stream, batch_mode_diverse(strat), sel, (int)h->N, (int)head,
                       eig, obj, h->N, ws, strat == SDPCUT_STRAT_COMB ? SDPCUT_BIG_M : 0.0, b.d_idx.get(), b.d_score.get());
    HIP_TRY(h, hipGetLastError());
    // what the assembly reads as the head of a point: the selection's, or -- the accepted entries are a head like any other -- the
    // filter's, its length in word 3 of the point's walk counts, which the assembly copies into the slice's header
    const int64_t *head_c4 = ws->counters, *head_idx = b.d_idx.get();
    int64_t head_c4_stride = ws_words;
    const double *head_score = b.d_score.get();
    if (F) {
        char *dv = (char *)b.d_div.get();
        DivPointsArgs A;
        A.pool = head; A.cap = cap; A.quota = sel_size; A.max_parallel = F->max_parallel; A.compare = F->max_parallel < 1.0 ? 1 : 0;
        A.sel_c4 = ws->counters; A.c4_stride = ws_words; A.idx = b.d_idx.get(); A.score = b.d_score.get(); A.idx_base = h->base; A.n_local = h->N;
        A.set5 = h->d_set_orig.get(); A.ks = h->d_k.get(); A.vars = b.d_pts.get(); A.vars_ld = n; A.nv = h->nb_vars; A.L = h->L; A.eig = eig; A.eig_ld = h->N;
        A.row_coef = (double *)(dv + dy.coef); A.row_lam = (double *)(dv + dy.lam); A.row_ks = (int32_t *)(dv + dy.ks);
        A.acc_idx = (int64_t *)(dv + dy.acc_idx); A.acc_score = (double *)(dv + dy.acc_score); A.info = (int64_t *)(dv + dy.info);
        A.sel_out = (int64_t *)b.div_sel.dev();
        if ((rc = launch_div_points(h, P, A))) return rc;
        head_c4 = A.info; head_c4_stride = 8; head_idx = A.acc_idx; head_score = A.acc_score;
    }
    for (int p = 0; p < P; ++p) std::memset(block + batch_point_offset(y, p), 0, 128);      // headers: counters, n_rows, nnz, give-up flag
    auto assemble = [&](int p_first, int count) -> int {
        return launch_round_csr_points(h, p_first, count, cap, ld, head_c4, head_c4_stride, head_idx, head_score, b.d_pts.get(), n, eig, h->N, b.d_agg.get(),
                                       BATCH_AGG_WORDS, b.pinned.dev(), (int64_t)y.slice, ++h->round_serial);
    };
    if ((rc = assemble(0, P))) return rc;
    HIP_TRY(h, sdpcut_sync(h));      // the one wait of the batch (a faulted kernel surfaces here as an error)

    std::vector<int> redo, again;
    const int64_t *selc = F ? (const int64_t *)b.div_sel.get() : nullptr;      // the filtered batch: the selection's counters of point p at selc + 8 p
    for (int p = 0; p < P; ++p) {
        const int64_t *hdr = (const int64_t *)(block + batch_point_offset(y, p));
        sdpcut_round_csr_t &o = out[p];
        int64_t n_head = 0;
        o.row_ld = ld;
        if (!rank_fast_finish(h, by_eff ? SDPCUT_STRAT_OPT : strat, sel_size, head, F ? selc + 8 * p : hdr, &n_head, &o.n_total, &o.new_strat, o.counters)) {
            redo.push_back(p);      // a void selection: the single-point call resolves it (tie split or full sort)
            continue;
        }
        if (F) {
            if (by_eff) o.new_strat = SDPCUT_STRAT_EFF;
            if (info) info[p].pool = n_head;
            if (n_head <= 0) continue;      // an empty ranking: an empty block
            if (info) { info[p].examined = hdr[0]; info[p].skipped_nonviolated = hdr[1]; info[p].rejected_parallel = hdr[2]; }
        }
        ++h->stat_rounds;
        o.cap = F ? (sel_size < n_head ? sel_size : n_head) : cap;
        o.n_out = F ? hdr[3] : n_head;
        if (hdr[10] && o.n_out > 0) again.push_back(p);
    }
    // a point whose row assembly gave up its bounded look-back (rows.hip): once more over the same head, like csr_assemble_wait (round.hip)
    for (int p : again) {
        int64_t *hdr = (int64_t *)(block + batch_point_offset(y, p));
        hdr[8] = hdr[9] = hdr[10] = 0;
        ++h->stat_fallbacks;
        if ((rc = assemble(p, 1))) return rc;
    }
    if (!again.empty()) {
        HIP_TRY(h, sdpcut_sync(h));
        for (int p : again)
            if (((const int64_t *)(block + batch_point_offset(y, p)))[10])
                return sdpcut_fail(h, SDPCUT_EHIP, std::string(F ? "round_csr_points_diverse" : "round_csr_points") + ": look-back of the row assembly timed out twice");
    }
    // (a redone point and an empty ranking of the filtered batch have no block: cap 0.  An answered point of the plain batch always
    // has o.cap == cap > 0: cap == 0 takes the loop route, batch_route.h)
    for (int p = 0; p < P; ++p) {
        sdpcut_round_csr_t &o = out[p];
        if (o.cap <= 0) continue;
        char *slot = block + batch_point_offset(y, p);
        const int64_t *hdr = (const int64_t *)slot;
        // (a ranking shorter than sel_size -- few violated candidates under strategy 1 -- has the block of its own length)
        if (o.cap < cap) csr_block_shrink(slot, cap, o.cap, ld, o.n_out, o.n_out > 0 ? hdr[8] : 0, o.n_out > 0 ? hdr[9] : 0);
        csr_out_from_block(slot, &o);
    }
    if (F) h->stat_diverse_points_fast += P - (int64_t)redo.size();
    for (int p : redo) {
        ++h->stat_points_redone;
        std::memset(out + p, 0, sizeof(*out));
        if (info) std::memset(info + p, 0, sizeof(*info));
        if ((rc = single(p))) return rc;
    }
    return SDPCUT_OK;
}

extern "C" {

int sdpcut_efficacy_points(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, double *eff_out, double *objpar_out,
                           double *escore_out)
{
    if (!h) return SDPCUT_EINVAL;
    return efficacy_points_impl(h, n_points, points, point_ld, eff_out, objpar_out, escore_out);
}

int sdpcut_round_csr_points_diverse(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, const double *lb, const double *ub,
                                    int64_t box_ld, int strat, int64_t sel_size, int64_t pool_size, double max_parallel, sdpcut_round_csr_t *out,
                                    sdpcut_diverse_info_t *info)
{
    if (!h) return SDPCUT_EINVAL;
    const BoxRows bx = {lb, ub, box_ld};
    const PointsFilter filter = {pool_size, max_parallel, info};
    const PointsRound R = {"sdpcut_round_csr_points_diverse", (lb || ub) ? &bx : nullptr, strat, sel_size, &filter};
    return round_points(h, R, n_points, points, point_ld, out);
}

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
    const PointsRound R = {"sdpcut_round_csr_points", nullptr, strat, sel_size, nullptr};
    return round_points(h, R, n_points, points, point_ld, out);
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
    const PointsRound R = {"sdpcut_round_csr_points_boxed", &bx, strat, sel_size, nullptr};
    return round_points(h, R, n_points, points, point_ld, out);
}

} // extern "C"
