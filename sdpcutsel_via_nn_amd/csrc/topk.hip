// Top-k selection on the device (k <= 16384) -- the fast path of the ranking.
//
// The reference sorts all N candidates (cut_select_qp.py:601, :653) but its caller consumes
// only the first sel_size <= 5000 (_SDP_CUTS_PER_ROUND_MAX, :37).  For such heads a full sort
// is wasted HBM traffic: this file finds the k-th largest key with an MSD radix select (eight
// 8-bit histogram passes over the u64 score images; candidates outside the class are masked
// to key 0), compacts the k selected (key, index) pairs -- every key above the threshold plus
// the lowest-index keys equal to it, exactly what a stable descending sort would keep -- and
// orders them by (key desc, index asc) with a counting sort spread over the chip.
//
// The passes stop as soon as the keys above the threshold bin plus the whole bin fit the sort
// buffers (<= 8192): that superset is compacted and sorted, and only its first k entries are
// emitted.  Spread-out scores need 2-3 of the 8 digits (the remaining launches return at once);
// masses of equal keys run to the last digit, where ties are cut by index.
//
// No host round trip anywhere: the last workgroup to finish a histogram pass (ticket counter)
// resolves that digit and publishes (prefix, need) for the next launch; the kernel boundary is
// the release/acquire.  Histogram cells and counters are written with device-scope atomics
// and read back by the resolving block with device-scope atomic loads (per-XCD L2s are not
// coherent for plain loads inside a launch).
//
// A round that scores for itself (sdpcut_select_round on a fresh point) does not run the first pass
// here: the score kernels count the leading digit of the class members' keys (score_mfma.hip; ScoreArgs::tk, score_launch.h)
// and tk_refine_kernel<true> starts at the second digit, building the keys from the scores as it
// reads them -- tk_keys_kernel and the key array are for selections over scores that exist already.
//
// Where things are.  topk_route.h decides the route (tk_route: plain values -> TkPlan, no HIP); this file is host only -- the
// workspace, the entry points, the tie split with its two tiny kernels -- and starts the kernels of the route files through the
// launchers of topk_launch.h:
//   route (TkRoute)                         file              kernels
//   SMALLSORT, SMALLSEL, SMALL              topk_small.hip    tk_smallsel_kernel<SORT>, tk_small_kernel
//   ONFLY, EMITTED, COOP, FUSED, DIGITS     topk_passes.hip   tk_keys_kernel / tk_prekeys_kernel (key pass of COOP, FUSED, DIGITS),
//                                                             tk_refine_kernel<ONFLY, EMIT>, tk_hist_kernel (DIGITS)
//   DIGITS, its compaction                  topk_compact.hip  tk_count_kernel, tk_write_kernel
//   the sort tail of all but SMALLSORT      topk_sort.hip     tk_countrank_kernel<TIE>, or tk_tilesort_kernel<TIE> and
//                                                             tk_mergerank_kernel<TIE> / tk_mergerank_big_kernel<TIE>
// Device code shared between them (TopkWs, resolve_digit, finish_pass, comp_less) and with the score kernels: topk_dev.h.
// The one-workgroup select-sort-emit algorithm (smallsel_body) is in topk_small_dev.h: tk_smallsel_kernel and the batched
// tk_points_kernel (points.hip, a workgroup per LP point) are its two hosts.

#include <utility>

#include "topk_launch.h"

// ------------------------------------------------------------------------------------------
int ensure_topk_ws(sdpcut_ctx *h)
{
    if (h->d_topk_ws.get()) return 0;
    HIP_TRY(h, h->d_topk_ws.reset(sizeof(TopkWs)));
    // first half: compacted selection, second half: the sorted tiles
    HIP_TRY(h, h->d_sel_key.reset(2 * TK_MAXK));
    HIP_TRY(h, h->d_sel_idx.reset(2 * TK_MAXK));
    // tk_countrank_kernel's per-entry words: zeroed once here, the wave that completes a word leaves it zero again
    HIP_TRY(h, h->d_rank_acc.reset(TK_LDSK));
    HIP_TRY(h, hipMemsetAsync(h->d_rank_acc.get(), 0, TK_LDSK * sizeof(unsigned long long), h->stream));
    const int rc = tk_refine_coresident(h, &h->tk_coresident);
    if (rc) return rc;
    if (h->tk_coresident < 1) h->fused_tail = false;      // (never on gfx950: 4 per CU by LDS) the launch-per-digit path has no waits
    return 0;
}

int topk_alt_ws(sdpcut_ctx *h, uint64_t **ptr, int *words)
{
    static_assert(sizeof(TopkWs) % 8 == 0, "TopkWs is zeroed in 8-byte words");
    if (!h->d_topk_ws_alt.get()) HIP_TRY(h, h->d_topk_ws_alt.reset(sizeof(TopkWs)));
    *ptr = (uint64_t *)h->d_topk_ws_alt.get();
    // (r5) lists too short for the fine histogram (it sits at the end of the struct) zero only what lies in front of it: the epilogue
    // of a round with a handful of cuts is a handful of workgroups, and every word is a store on its critical path
    static_assert(offsetof(TopkWs, pf_floor) % 8 == 0 && offsetof(TopkWs, pf_tab) > offsetof(TopkWs, pf_floor), "fine histogram last");
    *words = (int)((h->N >= SDPCUT_PF_MIN_N ? sizeof(TopkWs) : offsetof(TopkWs, pf_floor)) / 8);
    return 0;
}

// Enqueue the selection of the head of a ranking (no host synchronisation).
// mode: 1 feasibility, 2 optimality, 3 strong class.  min(k, class size) entries are written.
// *d_counters_out receives the device address of {class size, nb_violated, nb_positive, k_eff}.
int topk_begin(sdpcut_ctx *h, void **ws_out, uint64_t **keys_out)
{
    int rc = ensure_topk_ws(h);
    if (rc) return rc;
    rc = ensure_key_ws(h, h->N);
    if (rc) return rc;
    if (h->topk_alt_clean && h->d_topk_ws_alt.get()) {
        // the epilogue of the previous round zeroed the other workspace (stream-ordered): swap
        std::swap(h->d_topk_ws, h->d_topk_ws_alt);
        h->topk_alt_clean = false;
    } else {
        HIP_TRY(h, hipMemsetAsync(h->d_topk_ws.get(), 0, sizeof(TopkWs), h->stream));
    }
    if (ws_out) *ws_out = h->d_topk_ws.get();
    if (keys_out) *keys_out = h->d_key_a.get();
    return 0;
}

int64_t *topk_strong_counter(void *ws) { return ((TopkWs *)ws)->strong_rep; }

// the plan of a selection on this handle (topk_route.h)
static TkPlan plan_for(const sdpcut_ctx *h, int64_t n, int64_t k, int mode, int stage, bool prekeys, bool raw)
{
    TkRouteIn in;
    in.n = n; in.k = k; in.mode = mode; in.stage = stage;
    in.fused_tail = h->fused_tail; in.coop_launch = h->coop_launch; in.shard_rec = h->shard_rec != nullptr;
    in.prefilter = h->prefilter; in.pf_counted = h->pf_counted; in.tk_coresident = h->tk_coresident;
    in.prekeys = prekeys; in.raw = raw; in.count_rank = h->count_rank;
    in.emitted = h->emit_launched;
    return tk_route(in);
}

// may the score kernels count the leading digit for a head of k entries (ScoreFuse, stage 3)?  Asked BEFORE scoring, answered by
// the function the selection itself will be planned with (tk_fuse_ok, topk_route.h).
bool topk_fuse_ok(const sdpcut_ctx *h, int64_t k, bool comb)
{
    TkRouteIn in;
    in.n = h->N; in.k = k;
    in.fused_tail = h->fused_tail; in.coop_launch = h->coop_launch; in.shard_rec = h->shard_rec != nullptr;
    in.tk_coresident = h->tk_coresident;
    return tk_fuse_ok(in, comb);
}

// Enqueue a planned selection: the route's kernels, then the sort and the ranks.  prekeys: the keys are in h->d_key_a already.
static int topk_run(sdpcut_ctx *h, const TkPlan &p, const TkJob &j, bool prekeys)
{
    int rc = 0;
    // SDPCUT_OPT_INJECT_GIVEUP (tests), site 1: the void mark of an expired wait stands in the workspace before the route's kernels
    // start -- behind the zeroing of the workspace (topk_begin, stream order); neither the score kernels nor the key pass touch the
    // word.  Workgroups of tk_refine_kernel that reach a wait find the selection gone and leave, everything else runs to its end,
    // the sort tail emits nothing and the host discards the head: no kernel knows about the option.  The one-workgroup routes have
    // no bounded wait and no path behind one: they are no site.
    if (p.route > TK_ROUTE_SMALL && inject_take(h, 1)) {
        static const int64_t one = 1;
        HIP_TRY(h, hipMemcpyAsync(&j.ws->counters[4], &one, sizeof(one), hipMemcpyHostToDevice, h->stream));
    }
    switch (p.route) {
    case TK_ROUTE_SMALLSORT:
    case TK_ROUTE_SMALLSEL:
    case TK_ROUTE_SMALL:
        tk_small_launch(h, p, j);
        break;
    case TK_ROUTE_ONFLY:
    case TK_ROUTE_EMITTED:
        rc = tk_refine_launch(h, p, j);
        break;
    case TK_ROUTE_COOP:
    case TK_ROUTE_FUSED:
        prekeys ? tk_prekeys_launch(h, p, j) : tk_keys_launch(h, p, j);
        rc = tk_refine_launch(h, p, j);
        break;
    default:
        prekeys ? tk_prekeys_launch(h, p, j) : tk_keys_launch(h, p, j);
        tk_hist_launch(h, p, j);
        tk_compact_launch(h, p, j);
        break;
    }
    if (rc) return rc;
    if (p.route != TK_ROUTE_SMALLSORT) tk_sort_launch(h, p, j);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// stage 0: fresh selection; 1: the workspace has been handed out by topk_begin already (the score
// kernels left their strong count in it); 3: the score kernels also counted the leading digit of the keys
// and the violated / positive candidates (ScoreFuse; topk_fuse_ok).  mode TK_MODE_COMBAUTO: resolved by
// the first pass against `sel` (stages 1 and 3).
int topk_select_enqueue(sdpcut_ctx *h, int mode, int64_t k, double score_add, int64_t *d_idx_out,
                        double *d_score_out, const int64_t **d_counters_out, int stage, int64_t sel)
{
    const int64_t n = h->N;
    const TkPlan p = plan_for(h, n, k, mode, stage, false, false);
    if (p.err) return sdpcut_fail(h, p.err, p.msg);
    if (stage == 0) {
        const int rc = topk_begin(h, nullptr, nullptr);
        if (rc) return rc;
    }
    TopkWs *ws = (TopkWs *)h->d_topk_ws.get();
    const double *eig = (h->scored & SDPCUT_EIG) ? h->d_eig.get() : nullptr;
    const double *obj = (h->scored & SDPCUT_NN) ? h->d_obj : nullptr;
    const TkJob j = {ws, mode, n, k, sel, eig, obj, h->base, score_add, d_idx_out, d_score_out, 0, TK_MAXK};
    const int rc = topk_run(h, p, j, false);
    if (rc) return rc;
    if (d_counters_out) *d_counters_out = ws->counters;
    return 0;
}

// Head of a ranking over n PRECOMPUTED keys in h->d_key_a (0 = not in the class), ties by index:
// idx_out = entry index, val_out = the key's low 63 bits as a double; cnt as in topk_select_on_device.
int topk_select_keys_enqueue(sdpcut_ctx *h, int64_t n, int64_t k, int64_t *d_idx_out, double *d_val_out, const int64_t **d_counters_out)
{
    if (k < 1 || k > TK_MAXK || n < 1 || n > (int64_t)h->d_key_a.size()) return sdpcut_fail(h, SDPCUT_EINVAL, "top-k select: k / n out of range");
    // (always through the big-head merge: it is the one with the raw key output)
    const int64_t kk = k <= TK_LDSK ? TK_LDSK + 1 : k;
    const TkPlan p = plan_for(h, n, kk, TK_MODE_FEAS, 0, true, true);
    if (p.err) return sdpcut_fail(h, p.err, p.msg);
    int rc = topk_begin(h, nullptr, nullptr);
    if (rc) return rc;
    TopkWs *ws = (TopkWs *)h->d_topk_ws.get();
    const TkJob j = {ws, TK_MODE_FEAS, n, kk, 0, nullptr, nullptr, 0, 0.0, d_idx_out, d_val_out, 1, k};
    rc = topk_run(h, p, j, true);
    if (rc) return rc;
    *d_counters_out = ws->counters;
    return 0;
}

int topk_select_keys_on_device(sdpcut_ctx *h, int64_t n, int64_t k, int64_t *d_idx_out, double *d_val_out, int64_t cnt[5])
{
    const int64_t *d_cnt = nullptr;
    const int rc = topk_select_keys_enqueue(h, n, k, d_idx_out, d_val_out, &d_cnt);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(cnt, d_cnt, 5 * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return 0;
}

// ------------------------------------------------------------------------------------------
// The threshold tie group of the every-entry-visited combined ranking, cut by its SECONDARY key (r4).
//
// Mode COMBALL orders equal new scores by obj_improve, then index (the first stable sort of the reference,
// cut_select_qp.py:601, under its second, :625), so a group of equal keys that straddles position k cannot be cut by
// index.  As long as the whole group fits the sort buffers it is taken whole (resolve_digit); at a structured LP vertex --
// round 1 of every BoxQP run under the combined strategy with fewer than sel strong candidates: x = 0.5, X in {0, 0.5},
// thousands of candidates with the SAME -lambda_min -- it does not, the selection declares itself void (counters[4] = 2)
// and, until round 3, a rocPRIM sort of the full list answered.  Now: the void selection has left the threshold key T, the
// number of keys above it and the number `need` still wanted from the group in its workspace, and
//     head = [ every key > T, ordered (key, obj_improve, index) ]  ++  [ top `need` of the group by (obj_improve, index) ]
// -- two ordinary radix selections over precomputed keys: A keeps key > T (all of them are wanted: nothing to cut), B ranks
// the group by the image of obj_improve and cuts ITS ties by index, which is exactly the reference's order.  Hand-written
// path, no library sort, a few launches more than a normal round.
__global__ __launch_bounds__(TK_THREADS) void tk_tiekeys_kernel(int64_t n, uint64_t T, int part, const double *eig, const double *obj,
                                                                uint64_t *keys)
{
    for (int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * TK_THREADS) {
        const double o = obj[i];
        const uint64_t key = masked_key(TK_MODE_COMBALL, eig[i], o);
        keys[i] = part == 0 ? (key > T ? key : 0ull) : (key == T ? key_of(o) : 0ull);
    }
}

__global__ __launch_bounds__(TK_THREADS) void tk_fillscore_kernel(double *out, int64_t count, uint64_t T)
{
    const int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
    if (i < count) out[i] = score_of(T);
}

// head of a ranking over the n precomputed keys in h->d_key_a (0 = not in the class); tie: equal keys by obj_improve, then
// index (else by index).  Enqueued; *d_void receives the device address of the selection's void flag.
static int select_prekeys_enqueue(sdpcut_ctx *h, int64_t n, int64_t k, bool tie, int64_t *d_idx_out, double *d_score_out,
                                  const int64_t **d_void)
{
    const int mode = tie ? TK_MODE_COMBALL : TK_MODE_FEAS;
    const TkPlan p = plan_for(h, n, k, mode, 0, true, false);
    if (p.err) return sdpcut_fail(h, p.err, p.msg);
    const int rc = topk_begin(h, nullptr, nullptr);
    if (rc) return rc;
    TopkWs *ws = (TopkWs *)h->d_topk_ws.get();
    *d_void = &ws->counters[4];
    const TkJob j = {ws, mode, n, k, 0, nullptr, nullptr, h->base, 0.0, d_idx_out, d_score_out, 0, TK_MAXK};
    return topk_run(h, p, j, true);
}

// h->d_topk_ws holds a COMBALL selection for a head of k entries that declared itself void because of its threshold tie
// group (counters[4] == 2).  Writes the head (k_eff entries) to d_idx_out / d_score_out.
// -> 0 done; 1 not applicable (another kind of void: the caller takes its general path); < 0 error.
int topk_tie_split(sdpcut_ctx *h, int64_t k, int64_t *d_idx_out, double *d_score_out, int64_t *k_eff_out)
{
    const int64_t n = h->N;
    if (!h->d_topk_ws.get() || (h->scored & (SDPCUT_EIG | SDPCUT_NN)) != (SDPCUT_EIG | SDPCUT_NN) || k < 1 || k > TK_MAXK) return 1;
    const TopkWs *ws = (const TopkWs *)h->d_topk_ws.get();
    TkState st8;
    int64_t c[8];
    HIP_TRY(h, hipMemcpyAsync(&st8, &ws->state[8], sizeof(st8), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(c, ws->counters, sizeof(c), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    const int64_t k_eff = c[3], need = st8.need, above = k_eff - need;
    if (c[4] != 2 || c[6] != TK_MODE_COMBALL || need < 1 || above < 0 || k_eff > k) return 1;
    const uint64_t T = st8.prefix;
    int rc = ensure_key_ws(h, n);
    if (rc) return rc;
    const int64_t nb = (n + TK_THREADS - 1) / TK_THREADS;
    const int grid = (int)(nb < 4096 ? nb : 4096);
    int64_t void_a = 0, void_b = 0;
    const int64_t *d_void = nullptr;
    if (above > 0) {
        hipLaunchKernelGGL(tk_tiekeys_kernel, dim3(grid), dim3(TK_THREADS), 0, h->stream, n, T, 0, h->d_eig.get(), h->d_obj, h->d_key_a.get());
        rc = select_prekeys_enqueue(h, n, above, true, d_idx_out, d_score_out, &d_void);
        if (rc) return rc;
        HIP_TRY(h, hipMemcpyAsync(&void_a, d_void, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    }
    hipLaunchKernelGGL(tk_tiekeys_kernel, dim3(grid), dim3(TK_THREADS), 0, h->stream, n, T, 1, h->d_eig.get(), h->d_obj, h->d_key_a.get());
    rc = select_prekeys_enqueue(h, n, need, false, d_idx_out + above, d_score_out + above, &d_void);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(&void_b, d_void, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    hipLaunchKernelGGL(tk_fillscore_kernel, dim3((unsigned)((need + TK_THREADS - 1) / TK_THREADS)), dim3(TK_THREADS), 0, h->stream,
                       d_score_out + above, need, T);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, sdpcut_sync(h));
    if (void_a || void_b) return 1;      // a bounded wait expired (the GPU shared with a blocking kernel): the general path answers
    ++h->stat_tie_splits;
    if (k_eff_out) *k_eff_out = k_eff;
    return 0;
}

int topk_select_on_device(sdpcut_ctx *h, int mode, int64_t k, double score_add, int64_t *d_idx_out,
                          double *d_score_out, int64_t cnt[5])
{
    const int64_t *d_cnt = nullptr;
    int rc = topk_select_enqueue(h, mode, k, score_add, d_idx_out, d_score_out, &d_cnt, 0, 0);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(cnt, d_cnt, 5 * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return 0;
}
