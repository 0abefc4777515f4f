// SDPCUT_OPT_EXACT_HEAD (include/sdpcut.h): the head of an NN-ranked selection (strategies 2 and 4) ordered and reported by
// obj_improve in the REFERENCE's operation order.  The fast scores (score_mfma_body; within 1e-9 relative of the reference's
// bits, measured 2e-11) act as a filter:
//   zero band  (strategy 4) candidates whose fast score cannot decide the sign (exact_band.h) are re-scored and the exact values stand in
//              for the fast ones while the selection runs (d_obj is restored behind it): classes, regime and counters are
//              those of the exact signs;
//   selection  the ordinary top-k selection (topk.hip, routes unchanged) for a band of cap + margin entries;
//   re-score   exact_rescore_kernel over the band, arithmetic of score_simple_kernel;
//   re-rank    keys of the exact scores (keys.h images, masked_key), the sort tail of topk_sort.hip, first cap entries emitted;
//   verdict    the band rule of exact_band.h, evaluated on the device: ws->counters[4] = EXACT_VOID_BAND when the band does not
//              prove that it holds the exact head (the host retries once with the widest band, then returns the ordinary head),
//              EXACT_VOID_ZB when the zero band does not fit its buffer.
// Everything is enqueued; the caller's epilogue (or its copy of the counters) is the only host wait.
#include "exact_band.h"
#include "gather.h"
#include "libm_exp.h"
#include "topk_launch.h"

static_assert(EB_LDSK == TK_LDSK, "the band is ordered by the sort tail's LDS merge");

enum { EXACT_VOID_BAND = 3, EXACT_VOID_ZB = 4 };

struct ExactWs {
    int64_t zb_n;        // candidates found in the zero band (may exceed EB_ZB_MAX: then nothing is patched and the round gives up)
    int64_t zb_over;
    int64_t pad_[6];
};

// layout of h->d_exact
struct ExactBufs {
    ExactWs *xw;
    int64_t *zb_ids;      // [EB_ZB_MAX] global ids
    double *zb_old;       // [EB_ZB_MAX] what d_obj held
    double *zb_exact;     // [EB_ZB_MAX]
    int64_t *band_idx;    // [EB_LDSK] the approximate head of `band` entries
    double *band_sc;      // [EB_LDSK] its scores (not read)
    double *band_obj;     // [EB_LDSK] exact obj_improve by band position
};
static size_t exact_bytes() { return sizeof(ExactWs) + (size_t)EB_ZB_MAX * 24 + (size_t)EB_LDSK * 24; }
static ExactBufs exact_bufs(void *p)
{
    ExactBufs b;
    char *c = (char *)p;
    b.xw = (ExactWs *)c; c += sizeof(ExactWs);
    b.zb_ids = (int64_t *)c; c += (size_t)EB_ZB_MAX * 8;
    b.zb_old = (double *)c; c += (size_t)EB_ZB_MAX * 8;
    b.zb_exact = (double *)c; c += (size_t)EB_ZB_MAX * 8;
    b.band_idx = (int64_t *)c; c += (size_t)EB_LDSK * 8;
    b.band_sc = (double *)c; c += (size_t)EB_LDSK * 8;
    b.band_obj = (double *)c;
    return b;
}

// ------------------------------------------------------------------------------------------
// One pass over the fast scores: the zero band's members into a list; the strong candidates outside it counted for the
// device-resolved regime of the combined strategy (strong_rep of the selection's workspace; the members are added by
// exact_zb_patch_kernel once their exact sign is known).
__global__ __launch_bounds__(256) void exact_zb_scan_kernel(int64_t n, int64_t base, const double *obj, const double *eig, double max_elem,
                                                            ExactWs *xw, int64_t *zb_ids, int64_t *strong_rep)
{
    int64_t strong = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double o = obj[i];
        if (eb_zero_band(o, max_elem)) {
            const unsigned long long slot = atomicAdd((unsigned long long *)&xw->zb_n, 1ull);
            if (slot < (unsigned long long)EB_ZB_MAX) zb_ids[slot] = base + i;
        } else if (strong_rep && o > 0.0 && eig[i] < SDPCUT_NEG_EIGVAL) {
            ++strong;
        }
    }
    if (strong_rep) {
        for (int off = 32; off > 0; off >>= 1) strong += __shfl_xor((long long)strong, off);
        if ((threadIdx.x & 63) == 0 && strong)
            __hip_atomic_fetch_add((unsigned long long *)&strong_rep[blockIdx.x % TK_SREP], (unsigned long long)strong, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the exact scores of the zero band stand in for the fast ones until exact_finish_kernel puts those back
__global__ __launch_bounds__(256) void exact_zb_patch_kernel(int64_t base, double *obj, const double *eig, ExactWs *xw, const int64_t *zb_ids,
                                                             const double *zb_exact, double *zb_old, int64_t *strong_rep)
{
    const int64_t m = xw->zb_n;
    if (m > EB_ZB_MAX) {
        if (threadIdx.x == 0) xw->zb_over = 1;
        return;
    }
    for (int64_t j = threadIdx.x; j < m; j += 256) {
        const int64_t c = zb_ids[j] - base;
        zb_old[j] = obj[c];
        const double o = zb_exact[j];
        obj[c] = o;
        if (strong_rep && o > 0.0 && eig[c] < SDPCUT_NEG_EIGVAL)
            __hip_atomic_fetch_add((unsigned long long *)&strong_rep[j % TK_SREP], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ------------------------------------------------------------------------------------------
// obj_improve of listed candidates (mixed sizes k = 2..5) in the reference's operation order -- bit for bit what
// score_simple_kernel writes: no contraction, the host libm's exp, acc = acc + a * w with i ascending, then the bias, the output
// layer with j ascending, the epilogue negSM + y * max_elem.
// One wave (= one workgroup) per candidate: lane j owns hidden neuron j (the nets are 50 or 64 wide) and runs its own
// i-ascending chain, the activations of the previous layer are broadcast reads from LDS, the output layer is one serial
// j-ascending chain over them.  The order of operations of every neuron is the reference's; only WHERE the neurons of a layer
// run differs (64 lanes instead of one after the other).
struct ExactNets { NetDev net[SDPCUT_MAX_K + 1]; };

template <int K>
__device__ __forceinline__ double exact_obj_one(const NetDev &net, const int32_t *sp, const double *vars, const double *Q, int32_t nv,
                                                int64_t L, double (*act)[MAX_HIDDEN])
{
    constexpr int M = K * (K + 1) / 2;
    constexpr int DIN = K + M;
    const int lane = threadIdx.x;
    int32_t s[K];
#pragma unroll
    for (int a = 0; a < K; ++a) s[a] = sp[a];
    Cand<K> cd;
    gather_candidate<K>(cd, s, vars, Q, nv, L, true);
    double obj;
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int i = 0; i < DIN; ++i) {
            const double v = (i < K) ? cd.x[i < K ? i : 0] : cd.q[i >= K ? i - K : 0];
            if (lane == i) act[0][i] = (v - net.inmap[i]) * net.inmap[DIN + i] + net.ymin;
        }
        __syncthreads();
        int cur = 0, fan_in = DIN;
        for (int l = 0; l < net.n_hidden; ++l) {
            const double *W = net.raw_w[l], *b = net.raw_b[l];
            if (lane < net.width) {
                const double *Wj = W + (size_t)lane * fan_in;
                double acc = 0.0;
                for (int i = 0; i < fan_in; ++i) acc = acc + act[cur][i] * Wj[i];
                acc = acc + b[lane];
                act[cur ^ 1][lane] = 2.0 / (libm_exp(acc * -2.0) + 1.0) + -1.0;      // the host libm's exp: NNs.so's bits (libm_exp.h)
            }
            __syncthreads();
            cur ^= 1;
            fan_in = net.width;
        }
        const double *w = net.raw_w[net.n_hidden];
        double acc = 0.0;
        for (int j = 0; j < fan_in; ++j) acc = acc + act[cur][j] * w[j];
        acc = acc + net.b_out;
        const double y = (acc - net.y_ymin) / net.y_gain + net.y_xoffset;
        obj = cd.negSM;
        obj = obj + y * cd.max_elem;
    }
    __syncthreads();      // act is reused by the workgroup's next candidate
    return obj;
}

// ids: GLOBAL candidate ids; *d_count of them exist (at most max_count; nothing at all if *d_void != 0).
// out_pos[j] = obj_improve of ids[j]; out_full (optional, [N]) receives the same by candidate: the tie key of the sort tail.
__global__ __launch_bounds__(64) void exact_rescore_kernel(ExactNets nets, const int64_t *ids, int64_t base, const int64_t *d_count,
                                                           int64_t max_count, const int64_t *d_void, int64_t n, const int32_t *set_orig,
                                                           const int32_t *ks, const double *vars, const double *Q, int32_t nv, int64_t L,
                                                           double *out_pos, double *out_full)
{
    __shared__ double act[2][MAX_HIDDEN];
    if (d_void && *d_void) return;
    int64_t count = *d_count;
    if (count > max_count) count = max_count;
    for (int64_t j = blockIdx.x; j < count; j += gridDim.x) {
        const int64_t c = ids[j] - base;
        if (c < 0 || c >= n) continue;      // uniform: one candidate per workgroup
        const int k = ks[c];
        const int32_t *sp = set_orig + c * 5;
        double obj;
        switch (k) {
        case 2: obj = exact_obj_one<2>(nets.net[2], sp, vars, Q, nv, L, act); break;
        case 3: obj = exact_obj_one<3>(nets.net[3], sp, vars, Q, nv, L, act); break;
        case 4: obj = exact_obj_one<4>(nets.net[4], sp, vars, Q, nv, L, act); break;
        case 5: obj = exact_obj_one<5>(nets.net[5], sp, vars, Q, nv, L, act); break;
        default: continue;
        }
        if (threadIdx.x == 0) {
            out_pos[j] = obj;
            if (out_full) out_full[c] = obj;
        }
    }
}

// ------------------------------------------------------------------------------------------
// Re-rank, first half: the band's (exact key, candidate) pairs into the sort tail's input.  The mode is the one the selection
// resolved (ws->mode); the signs of the exact scores are those the selection saw (zero band patched).
__global__ __launch_bounds__(256) void exact_keys_kernel(const TopkWs *ws, const int64_t *band_idx, int64_t base, int64_t n, const double *eig,
                                                         const double *band_obj, uint64_t *sel_key, uint32_t *sel_idx)
{
    if (ws->counters[4]) return;
    int64_t nb = ws->counters[3];
    if (nb > EB_LDSK) nb = EB_LDSK;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nb) return;
    const int64_t c = band_idx[j] - base;
    const bool ok = c >= 0 && c < n;
    const int mode = (int)ws->mode;
    sel_key[j] = ok ? masked_key(mode, eig ? eig[c] : 0.0, band_obj[j]) : 0ull;
    sel_idx[j] = ok ? (uint32_t)c : 0u;
}

// Second half (one workgroup): the verdict of the band rule, the counts the sort tail and the epilogue read (n_sel = band,
// counters[3] = entries of the head), and the fast scores of the zero band back into d_obj.
__global__ __launch_bounds__(256) void exact_finish_kernel(TopkWs *ws, ExactWs *xw, int64_t cap, int64_t band, int64_t n, int64_t base,
                                                           const int64_t *band_idx, double *obj, const double *eig, double max_elem,
                                                           const int64_t *zb_ids, const double *zb_old)
{
    if (threadIdx.x == 0) {
        if (xw && xw->zb_over) {
            ws->counters[4] = EXACT_VOID_ZB;
        } else if (!ws->counters[4]) {
            const int64_t nb = ws->counters[3], cls = ws->counters[0];
            const int mode = (int)ws->mode;
            bool holds = false;
            if (cls > band && nb == band && band > cap && cap >= 1) {
                const int64_t ca = band_idx[cap - 1] - base, cb = band_idx[band - 1] - base;
                if (ca >= 0 && ca < n && cb >= 0 && cb < n) {
                    const double sa = score_of(masked_key(mode, eig ? eig[ca] : 0.0, obj[ca]));
                    const double sb = score_of(masked_key(mode, eig ? eig[cb] : 0.0, obj[cb]));
                    holds = eb_band_holds(sa, sb, max_elem, mode == TK_MODE_COMBALL);
                }
            }
            if (eb_decide(n, cls, band, holds) != EB_EXACT) {
                ws->counters[4] = EXACT_VOID_BAND;
            } else {
                ws->n_sel = nb;
                ws->counters[3] = nb < cap ? nb : cap;
            }
        }
        if (ws->counters[4]) {      // void (the selection's own reasons included): the sort tail emits nothing
            ws->n_sel = 0;
            ws->counters[3] = 0;
        }
    }
    __syncthreads();
    if (!xw) return;      // strategy 2: no zero band, nothing stands in
    const int64_t m = xw->zb_over ? 0 : xw->zb_n;
    for (int64_t j = threadIdx.x; j < m; j += 256) obj[zb_ids[j] - base] = zb_old[j];
}

// the same restore alone: enqueued when the host cannot enqueue the rest of the head behind exact_zb_patch_kernel
__global__ __launch_bounds__(256) void exact_restore_kernel(const ExactWs *xw, int64_t base, double *obj, const int64_t *zb_ids,
                                                            const double *zb_old)
{
    const int64_t m = xw->zb_over ? 0 : xw->zb_n;
    for (int64_t j = threadIdx.x; j < m; j += 256) obj[zb_ids[j] - base] = zb_old[j];
}

// ------------------------------------------------------------------------------------------
int exact_head_applies(const sdpcut_ctx *h, int strat)
{
    return h->exact_head && !h->exact_suspended && (strat == SDPCUT_STRAT_OPT || strat == SDPCUT_STRAT_COMB);
}

int64_t exact_first_band(const sdpcut_ctx *h, int64_t cap) { return eb_first_band(h->N, cap); }
int64_t exact_widest_band(const sdpcut_ctx *h) { return h->N < EB_LDSK ? h->N : EB_LDSK; }

static int ensure_exact_ws(sdpcut_ctx *h, bool full)
{
    if (!h->d_exact.get()) {
        HIP_TRY(h, h->d_exact.reset(exact_bytes()));
        HIP_TRY(h, hipMemsetAsync(h->d_exact.get(), 0, exact_bytes(), h->stream));
    }
    return full ? grow(h, h->d_obj_exact, (size_t)h->N) : 0;
}

// Enqueue the exact head of `cap` entries (strategy 2 or 4; the measures are scored already) through a band of `band` entries into
// d_idx_out / d_score_out.  *d_c4 = the selection's counters as every other selection leaves them, [3] = entries written,
// [4] = 0 or why the head is void (EXACT_VOID_*, or the selection's own reasons).  No host wait.
int exact_head_enqueue(sdpcut_ctx *h, int strat, int64_t sel_size, int64_t cap, int64_t band, int64_t *d_idx_out, double *d_score_out,
                       const int64_t **d_c4)
{
    const int64_t n = h->N;
    const bool comb = strat == SDPCUT_STRAT_COMB;
    if (cap < 1 || band < cap || band > EB_LDSK || band > n) return sdpcut_fail(h, SDPCUT_EINVAL, "exact head: band out of range");
    for (int k = 2; k <= SDPCUT_MAX_K; ++k)
        if (h->bucket[k].n && !h->net[k].set) return sdpcut_fail(h, SDPCUT_ESTATE, "exact head: no network for a size class of the list");
    int rc = ensure_exact_ws(h, comb);
    if (rc) return rc;
    const ExactBufs B = exact_bufs(h->d_exact.get());
    void *wsv = nullptr;
    rc = topk_begin(h, &wsv, nullptr);
    if (rc) return rc;
    TopkWs *ws = (TopkWs *)wsv;
    int64_t *strong = comb ? topk_strong_counter(wsv) : nullptr;
    const double me = eb_max_elem_bound(h->q_absmax);
    const double *eig = comb ? h->d_eig.get() : nullptr;
    ExactNets nets;
    for (int k = 0; k <= SDPCUT_MAX_K; ++k) nets.net[k] = h->net[k].dev;
    const int mode = comb ? TK_MODE_COMBAUTO : TK_MODE_OPT;
    const int64_t sel = sel_size < n ? sel_size : n;
    TkRouteIn in;
    in.n = band; in.k = cap; in.mode = mode; in.stage = 1; in.prekeys = true;
    in.fused_tail = h->fused_tail; in.tk_coresident = h->tk_coresident; in.count_rank = h->count_rank;
    const TkPlan p = tk_route(in);      // (only the sort tail's grid and tie rule are read)
    if (p.err) return sdpcut_fail(h, p.err, p.msg);
    // ---- zero band.  Combined strategy only: under strategy 2 no class depends on the sign of obj_improve (the one thing that
    // does, nb_positive, is then the fast scores' count, as with the option off).
    if (comb) {
        HIP_TRY(h, hipMemsetAsync(B.xw, 0, sizeof(ExactWs), h->stream));
        const int64_t nb = (n + 255) / 256;
        const int g_scan = (int)(nb < 4 * h->n_cu ? nb : 4 * h->n_cu);
        hipLaunchKernelGGL(exact_zb_scan_kernel, dim3(g_scan), dim3(256), 0, h->stream, n, h->base, h->d_obj, eig, me, B.xw, B.zb_ids, strong);
        hipLaunchKernelGGL(exact_rescore_kernel, dim3(EB_ZB_MAX), dim3(64), 0, h->stream, nets, B.zb_ids, h->base, &B.xw->zb_n,
                           (int64_t)EB_ZB_MAX, (const int64_t *)nullptr, n, h->d_set_orig.get(), h->d_k.get(), h->d_vars.get(), h->d_Q.get(), h->nb_vars, h->L,
                           B.zb_exact, (double *)nullptr);
        hipLaunchKernelGGL(exact_zb_patch_kernel, dim3(1), dim3(256), 0, h->stream, h->base, h->d_obj, eig, B.xw, B.zb_ids, B.zb_exact,
                           B.zb_old, strong);
        HIP_TRY(h, hipGetLastError());
    }
    // from here on d_obj may hold stand-in values: an error return enqueues their restore first (d_obj is never left written)
    auto undo = [&](int code) {
        if (comb) hipLaunchKernelGGL(exact_restore_kernel, dim3(1), dim3(256), 0, h->stream, B.xw, h->base, h->d_obj, B.zb_ids, B.zb_old);
        return code;
    };
    // ---- the band: the ordinary selection (regime of the combined strategy resolved on the device from the strong count above)
    rc = topk_select_enqueue(h, mode, band, 0.0, B.band_idx, B.band_sc, d_c4, 1, sel);
    if (rc) return undo(rc);
    // ---- re-score, re-rank
    hipLaunchKernelGGL(exact_rescore_kernel, dim3((unsigned)(band < 4096 ? band : 4096)), dim3(64), 0, h->stream, nets, B.band_idx, h->base, &ws->counters[3], band,
                       &ws->counters[4], n, h->d_set_orig.get(), h->d_k.get(), h->d_vars.get(), h->d_Q.get(), h->nb_vars, h->L, B.band_obj,
                       comb ? h->d_obj_exact.get() : (double *)nullptr);
    hipLaunchKernelGGL(exact_keys_kernel, dim3((unsigned)((band + 255) / 256)), dim3(256), 0, h->stream, ws, B.band_idx, h->base, n, eig,
                       B.band_obj, h->d_sel_key.get(), h->d_sel_idx.get());
    if (hipGetLastError() != hipSuccess) return undo(sdpcut_fail(h, SDPCUT_EHIP, "exact head: launch of the re-score failed"));
    hipLaunchKernelGGL(exact_finish_kernel, dim3(1), dim3(256), 0, h->stream, ws, comb ? B.xw : (ExactWs *)nullptr, cap, band, n, h->base,
                       B.band_idx, h->d_obj, eig, me, B.zb_ids, B.zb_old);
    HIP_TRY(h, hipGetLastError());
    // (a void head has n_sel = 0: the tail emits nothing)
    const TkJob j = {ws, mode, band, cap, sel, eig, h->d_obj, h->base, comb ? SDPCUT_BIG_M : 0.0, d_idx_out, d_score_out, 0, TK_MAXK,
                     h->d_obj_exact.get()};
    tk_sort_launch(h, p, j);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// What the host does with the counters of an exact head (c4 as the epilogue / a copy delivers them):
// 0 exact, EB_RETRY: enqueue again with exact_widest_band, EB_GIVE_UP: serve the ordinary head.
int exact_head_verdict(sdpcut_ctx *h, const int64_t c4[7], int64_t band)
{
    if (!c4[4]) return EB_EXACT;
    if (c4[4] == EXACT_VOID_BAND && band < exact_widest_band(h)) return EB_RETRY;
    return EB_GIVE_UP;
}
