// Shared host-side declarations of libsdpcut_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <functional>
#include <string>
#include <vector>

#include "../../include/sdpcut.h"
#include "bufs.h"          // DevBuf, HostBuf: the owners of every device and pinned allocation
#include "net_pack.h"      // MAX_HIDDEN, MAX_LAYERS, SDPCUT_INPUT_CLAMP, net_pack
#include "round_layout.h"  // RowsLayout, CsrLayout

#define SDPCUT_NEG_EIGVAL (-1e-15) /* _THRES_NEG_EIGVAL, cut_select_qp.py:24 */
#define SDPCUT_BIG_M 1000.0        /* _BIG_M, cut_select_qp.py:26 */

// Device-side description of one trained MLP (k = 2..5); passed to kernels by value.
struct NetDev {
    int d_in;
    int n_hidden;          // hidden (tansig) layers
    int width;             // hidden width (all hidden layers equal: 64 or 50)
    int s0, sh;            // k-steps (of 4) of the first / the other hidden layers
    // The MFMA kernel's copies of the hidden-layer weights and biases are pre-scaled by -1/4: the
    // accumulators then hold y/8 = -n/4 of tansig's exp(-2n) = exp(y) directly (exact: scaling by
    // a power of two commutes with every rounding of the dot product), one multiply less per
    // activation.
    const double *wfrag;   // MFMA A-fragments (x -1/4): layer-major, then [t][s][lane]
    const double *wtail;   // (x -1/4) [layer][4][64]: rows 48..51 of each hidden layer (VALU tail of the MFMA kernel)
    const double *bias_q;  // (x -1/4) [n_hidden][64] zero padded
    const double *wvalu;   // scalar-operand packing: layer-major, then [j/8][i][j%8], zero padded
    const double *bias;    // [n_hidden][64] zero padded
    const double *wout;    // [64] zero padded output weights
    const double *inmap;   // xoffset[d_in] | gain[d_in]
    const double *raw_w[MAX_LAYERS]; // row-major [out][in] (simple kernel)
    const double *raw_b[MAX_LAYERS];
    double ymin, b_out, y_ymin, y_gain, y_xoffset;
    // every pre-activation is provably below the tansig's overflow clamp when the mapped inputs lie in
    // [-SDPCUT_INPUT_CLAMP, SDPCUT_INPUT_CLAMP], AND the network's mapping sends the input domain (x in [0, 1], |q| <= 1/k)
    // into that interval (net_pack.h, sdpcut_set_network): the MFMA kernel then clamps the 9..20 inputs of a candidate once
    // instead of its 150..256 activations, and that clamp changes nothing on the domain
    int unclamped_ok;
    // The fp32 filter of the skipping kernel (score_mfma.hip, stage F; net_pack.h has the packing and the derivation of the margin).
    // filter_ok: clamp-free, the shipped 3-variable shape, margin below FILTER_MARGIN_CUTOFF; the pointers are set only then.
    int filter_ok;
    double filter_margin;      // proven bound on |y32 - y64| of the unmapped output for mapped inputs inside filter_box
    const double *filter_box;  // [d_in][2]: lo, hi of every mapped input; a candidate outside bypasses the filter
    const float *f32_in;       // (x -2 log2 e) input-layer A-fragments of v_mfma_f32_16x16x4_f32: [t][lane] float4, component = k-step
    const float *f32_hid;      // (x -2 log2 e) hidden-layer A-fragments: [layer - 1][t][tk][lane] float4, component i = k-step (tk, i)
    const float *f32_bias;     // (x -2 log2 e) [n_hidden][64] zero padded
    // the margin per candidate, min(filter_margin, (S (1 + 2^-9) + filter_c0) (1 + 2^-10)) with S = sum_j f32_g[j] (1 - a_j^2) over
    // the last hidden layer's fp32 activations (net_pack.h: net_filter_slope_terms)
    const float *f32_g;        // [64] zero padded, neuron order
    double filter_c0;
};

struct Bucket {
    int64_t n = 0;
    DevBuf<int32_t> d_set;      // SoA [k][n]
    DevBuf<int32_t> d_orig;     // [n] local candidate index (position in caller's list)
};

struct NetHost {
    bool set = false;
    NetDev dev{};
    DevBuf<char> d_blob;        // one allocation behind all device pointers of dev (doubles, then the filter's floats)
};

// the resident training set of one candidate size and the workspace of its gradient evaluations (train.hip)
struct TrainData {
    int64_t count = 0;
    DevBuf<double> d_in;        // [count][k(k+3)/2], the layout of sdpcut_nn_batch
    DevBuf<double> d_t;         // [count]
};

// a fused round between its two halves (round.hip: round_begin / round_end)
struct PendingRound {
    bool active = false, csr = false, fast_tried = false;
    bool skipped = false;          // its scoring launch ran the MLP for violated candidates only (SDPCUT_OPT_SKIP_NONVIOLATED)
    int strat = 0;
    uint32_t view = 0;             // strategies 3 and 6: the measure (SDPCUT_SDP / SDPCUT_EFF) whose MeasureAsObj view the round was begun in and is ended in
    int32_t ld = 0;
    int64_t sel_size = 0, cap = 0, serial = 0;
    int64_t exact_band = 0;        // > 0: the enqueued head is an exact one (SDPCUT_OPT_EXACT_HEAD) through a band of this many entries
};

// every entry point that touches the handle's scores, staging or pinned block refuses to run between the two halves of a round
// (fused: round_csr_begin / _end; sharded: shard_finish_enqueue / _wait -- their kernels are still writing d_stage and the pinned block)
#define SDPCUT_NO_PENDING(h)                                                                                              \
    do {                                                                                                                  \
        if ((h)->pend.active)                                                                                             \
            return sdpcut_fail((h), SDPCUT_ESTATE, "a round begun with sdpcut_round_csr_begin is pending on this handle: end it first"); \
        if ((h)->shard_pending_serial)                                                                                    \
            return sdpcut_fail((h), SDPCUT_ESTATE, "a sharded round enqueued with sdpcut_shard_finish_enqueue is pending on this handle: " \
                                                   "sdpcut_shard_finish_wait first");                                    \
    } while (0)

// what a batch of LP points needs beside the handle's single-point state (points.hip); everything grows on demand
struct PointsBufs {
    HostBuf stage{true};                            // mapped staging of the points [P][L + n] (a boxed batch: and its (l | d) rows behind them)
    DevBuf<double> d_pts;                           // [P][L + n]
    DevBuf<double> d_eig, d_obj;                    // [P][N]; grown together
    DevBuf<char> d_ws;                              // TopkWs[P]: selection state and counters of every point
    DevBuf<int64_t> d_idx;                          // [P][cap] heads; grown together with d_score
    DevBuf<double> d_score;
    DevBuf<uint64_t> d_agg;                         // [P][BATCH_AGG_WORDS] look-back words of the row assembly
    HostBuf pinned{true};                           // the batch block (batch_route.h: batch_layout)
    // a boxed batch (sdpcut_*_points_boxed): its (l | d) rows travel behind the points in the staging block
    DevBuf<double> d_box_ld;                        // [P][2 n]
    DevBuf<double> d_Q_box, d_vars_box;             // [P][L] Q' and [P][L + n] transformed points (box.hip: box_points_kernel); grown together
    // efficacy over a batch (sdpcut_efficacy_points, the batched strategy-6 round): eff | objpar | escore, [P][N] each
    DevBuf<double> d_eff;
    // the filtered batch (sdpcut_round_csr_points_diverse): pool rows, accepted heads and walk counts of every point in one device
    // allocation; the selection counters of every point in mapped host memory
    DevBuf<char> d_div;
    HostBuf div_sel{true};                          // [P][8] int64
};

struct sdpcut_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev_switch = nullptr;      // sdpcut_set_stream: orders the new stream behind the old one; created by the first switch
    // the small size classes of a mixed cover are scored on side streams next to the largest one (launch_score)
    bool one_launch = true;      // SDPCUT_OPT_ONE_LAUNCH: the size classes of a mixed list in one launch (score_mfma_all_kernel)
    int side_streams = 0;        // SDPCUT_OPT_SIDE_STREAMS: 0 off (default since r4: no code path picked by a timing), 1 on, 2 measured once per candidate list (side_choice)
    int side_choice = -1;        // -1 not measured yet, 0 one after the other, 1 side streams
    float side_ms[2] = {0.f, 0.f};
    hipStream_t side_stream[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    std::string err;
    int kernel_variant = SDPCUT_KERNEL_MFMA;
    bool fuse_keys = true;         // SDPCUT_OPT_FUSE_KEYS (see include/sdpcut.h)
    bool auto_regime = true;       // SDPCUT_OPT_AUTO_REGIME
    bool fused_tail = true;        // SDPCUT_OPT_FUSED_TAIL
    bool eig_kernel = true;        // SDPCUT_OPT_EIG_KERNEL: eigenvalue-only launches run eig_only_kernel (eig.hip)
    bool pf_counted = false;       // the scoring launches of the current round all counted the fine histogram (launch_score)
    bool prefilter = true;         // SDPCUT_OPT_PREFILTER: fine histogram in the score kernels, direct selection (topk_dev.h)
    DevBuf<unsigned long long> d_stats;      // device counters that outlive a round: [0] direct selections, [1..3] its diagnostics, [4] nb_violated of a skipped sharded head, [5] fp64 evaluations of a filtering launch, [6] selections from the emitted list
    bool coop_launch = false;      // SDPCUT_OPT_COOP_LAUNCH: cooperative launch of the kernels with grid barriers (+20 us per round)
    int64_t stat_rounds = 0, stat_fallbacks = 0, stat_tie_splits = 0;   // sdpcut_get_stat
    // SDPCUT_OPT_INJECT_GIVEUP (tests): launches of inject_site (1 selection, 2 row-assembly look-back) -- inject_skip of them pass,
    // the inject_count after them are hit (inject_take below); stat_injected counts the hits
    int inject_site = 0, inject_skip = 0, inject_count = 0;
    int64_t stat_injected = 0;        // SDPCUT_STAT_INJECTED
    int64_t stat_points_redone = 0;   // SDPCUT_STAT_POINTS_REDONE
    int64_t stat_diverse_points_fast = 0;   // SDPCUT_STAT_DIVERSE_POINTS_FAST
    int64_t stat_tri_points_fast = 0;       // SDPCUT_STAT_TRI_POINTS_FAST
    int64_t stat_node_eval_points = 0;      // SDPCUT_STAT_NODE_EVAL_POINTS
    PointsBufs pts;                   // sdpcut_score_points / sdpcut_round_csr_points
    // SDPCUT_OPT_EXACT_HEAD (exact_head.hip): NN-ranked heads ordered and reported by reference-order obj_improve
    bool exact_head = false;
    bool exact_suspended = false;  // a round that gave up is being served by the ordinary path
    int64_t stat_exact_last = 0, stat_exact_gave_up = 0, stat_exact_retries = 0;
    double q_absmax = 0.0;         // max |Q_arr| of the instance (bound on every candidate's max_elem, exact_band.h)
    DevBuf<char> d_exact;          // zero band, band ids and exact scores (exact_head.hip: ExactBufs)
    DevBuf<double> d_obj_exact;    // [N] exact obj_improve of the band's members by candidate: tie key of the every-entry-visited sort
    int timing = 0;                // 0 off, 1 events around the score kernel, 2 also around the ranking
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool timed_score = false;      // ev[0] / ev[1] were attached to the last score launch
    float ms_score = 0.f, ms_rank = 0.f;
    int n_cu = 256;

    int32_t nb_vars = 0;
    int64_t L = 0;
    DevBuf<double> d_Q;         // [L]
    DevBuf<double> d_vars;      // [L + n]
    // set by sdpcut_shard_head_device around its selection: the sort's last kernel also writes the
    // record header and the padding (topk_sort.hip, tk_mergerank_kernel)
    int64_t *shard_rec = nullptr;
    int64_t shard_rec_count = 0, shard_rec_len = -1;
    bool have_point = false;
    // node box (box.hip, sdpcut_set_box): the tables SDPCUT_NN / SDPCUT_SDP are computed from while a box is set
    bool box_set = false;
    DevBuf<double> d_box_ld;       // [2 n]: l | d = u - l
    DevBuf<double> d_Q_box;        // [L] Q'
    DevBuf<double> d_vars_box;     // [L + n] the transformed point; follows d_vars in stream order (box_after_point)
    std::vector<double> box_lb, box_ub;

    int64_t N = 0, base = 0;
    int32_t row_len_max = 5;       // k + k(k+1)/2 of the largest candidate size present
    Bucket bucket[SDPCUT_MAX_K + 1];
    DevBuf<int32_t> d_set_orig;    // [N][5] padded, caller order
    DevBuf<int32_t> d_k;           // [N]
    DevBuf<double> d_eig;          // [N] caller order
    // the optimality array every ranking reads, [N] caller order: obj_own's, or -- inside a MeasureAsObj view -- a measure's
    double *d_obj = nullptr;
    DevBuf<double> obj_own;
    // SDPCUT_SDP (exact_sdp.hip): exact optimality measure and its duality gap, [N] caller order, allocated by the first scoring
    DevBuf<double> d_sdp, d_sdp_gap;
    DevBuf<unsigned long long> d_sdp_unconverged;      // candidates of the last exact solve that stopped at the iteration cap
    // SDPCUT_EFF (efficacy.hip): efficacy of the emitted row, its objective parallelism and the ranking score eff + w objpar, [N]
    // caller order, one allocation made by the first scoring and freed with the candidates
    DevBuf<double> d_eff;          // the allocation; d_objpar and d_escore point into it
    double *d_objpar = nullptr, *d_escore = nullptr;
    DevBuf<double> d_lpobj;        // [L + n] LP objective vector (sdpcut_set_objective) or NULL; belongs to the instance
    double lpobj_norm = 0.0;       // its 2-norm, computed once when it is set
    DevBuf<double> d_lpobj_dense;      // [n][n] the objective's a_ij in both triangles (node_eval.hip), n <= 1024; freed with d_lpobj
    bool lpobj_dense_ok = false;       // ... and it is the table of the vector in d_lpobj (built by the first node evaluation after a set_objective)
    double eff_w = 0.0;            // sdpcut_set_efficacy_weight
    bool exact_sdp = false;        // SDPCUT_OPT_EXACT_SDP: strategy 3 is accepted
    uint32_t scored = 0;
    // SDPCUT_OPT_SKIP_NONVIOLATED (score_mfma_skip_kernel): 0 never, 1 lists score_plan cuts into strips of 64, 2 every list
    int skip_nonviolated = 1;
    bool skip_launched = false;    // the last launch_score ran the skipping kernel
    // SDPCUT_OPT_FP32_FILTER (score_mfma_filter_kernel): the skipping launch filters in fp32 where the network qualifies
    bool fp32_filter = true;
    bool filter_launched = false;  // ... and it was the filtering one
    // SDPCUT_OPT_EMIT_HEAD: the skipping launch of a round whose regime the device resolves appends its strong members (key, index)
    // to a list in d_key_a -- a stage-3 selection has no key array -- and the selection reads that list (TK_ROUTE_EMITTED)
    bool emit_head = true;
    int64_t emit_cap_opt = 0;      // SDPCUT_OPT_EMIT_CAP (tests): > 0 caps the list
    bool emit_launched = false;    // the last launch_score emitted ...
    int64_t emit_cap = 0;          // ... into a list of this many entries in d_key_a: (key, index) pairs of two 64-bit words
    // SDPCUT_STAT_NN_EVALUATED of the last launch that ran the network: 0 everybody (nn_eval_n), 1 the violated candidates
    // (nn_eval_n - SDPCUT_STAT_NN_SKIPPED), 2 the filter's survivors (d_stats[5], left there by the selection's first kernel)
    int nn_eval_mode = 0;
    int64_t nn_eval_n = 0;
    // d_obj holds the optimality measure of a SUPERSET OF THE STRONG candidates only (a skipped round in its strong regime): of the
    // violated ones, or -- behind the fp32 filter -- of the violated ones the filter could not prove non-positive.  While set,
    // `scored` carries no SDPCUT_NN -- whoever needs the measure scores it like a missing one, which completes the array
    // (launch_score counts that) -- and SDPCUT_STAT_SCORED still reports the bit.  Cleared with `scored`.
    bool obj_partial = false;
    // SDPCUT_STAT_NN_SKIPPED: what the last scoring launch skipped (0 after one that scored everybody; reset with the list).  A
    // sharded head has no host wait: its selection's nb_violated is copied on the stream into d_stats[4] (which outlives every
    // workspace) and the stat is nn_skipped_n - d_stats[4], read when asked for (nn_skipped_on_device).
    int64_t stat_nn_skipped = 0, nn_skipped_n = 0;
    bool nn_skipped_on_device = false;
    int64_t stat_nn_completions = 0;   // SDPCUT_STAT_NN_COMPLETIONS
    int64_t last_total = -1;       // length of the last ranking (-1: none), see sdpcut_rank_fetch

    NetHost net[SDPCUT_MAX_K + 1];

    // ranking workspace (sized to N by ensure_rank_ws)
    int64_t ws_n = 0;              // entries the full-list arrays (all but d_key_a) hold (ensure_rank_ws)
    DevBuf<uint64_t> d_key_a, d_key_b;   // d_key_a grows on its own (ensure_key_ws)
    DevBuf<uint32_t> d_val_a, d_val_b;   // 2 n entries: 8 B per entry of the list, also used as u64 by the merge
    DevBuf<int32_t> d_flag, d_scan;
    DevBuf<int64_t> d_counters;    // [8]
    DevBuf<char> d_tmp;            // rocPRIM's temporary storage; tmp_bytes of it are what the primitives asked for
    size_t tmp_bytes = 0;
    // top-k select workspace (topk.hip)
    DevBuf<char> d_topk_ws;
    int64_t tk_coresident = 256;   // workgroups of tk_refine_kernel resident at once (occupancy x CUs), set with the workspace
    DevBuf<char> d_topk_ws_alt;    // second workspace: zeroed by the epilogue of a round for the next one
    bool topk_alt_clean = false;   // d_topk_ws_alt has been (stream-ordered) zeroed and may be swapped in
    DevBuf<uint64_t> d_sel_key;
    DevBuf<uint32_t> d_sel_idx;
    bool count_rank = true;        // SDPCUT_OPT_COUNT_RANK: the sort tail ranks by counting in one launch (tk_countrank_kernel)
    DevBuf<unsigned long long> d_rank_acc;      // [TK_LDSK] rank sum | arrivals of every compacted entry; zero between launches
    // triangle inequalities (tri.hip)
    DevBuf<int32_t> d_tri;             // [T][3]
    DevBuf<uint8_t> d_tri_dense3;      // [T] density == 3
    int64_t n_tri = 0;
    bool tri_ready = false;            // sdpcut_tri_preprocess has run (n_tri = 0 is a list too)
    void *tri_pts = nullptr;           // triangle rounds over a batch of points (tri_points.hip: TriPointsBufs); allocated by the first call
    void *node_eval = nullptr;         // node evaluation (node_eval.hip: NodeEvalBufs): staging and result block; allocated by the first call
    std::vector<int32_t> tri_host;
    std::vector<uint8_t> tri_dense_host;
    // small staging
    DevBuf<char> d_stage;
    HostBuf pinned{true};          // host block of sdpcut_select_round (written by the device, one sync per round)
    // sdpcut_set_point: pinned staging copy of the caller's LP point and the event of its transfer
    HostBuf point_stage{true};
    bool point_inflight = false;   // a transfer out of point_stage may still be running
    int64_t round_serial = 0;      // completion word of the fused round (round_rows_kernel -> pinned header)
    DevBuf<uint32_t> d_done_ticket;      // completion ticket, then the look-back words of the row assemblies (ensure_round_sync)
    PendingRound pend;
    TrainData train[SDPCUT_MAX_K + 1];   // sdpcut_train_set_data; independent of instance, candidates, point and networks
    DevBuf<double> d_train_ws;     // parameters | per-workgroup partial sums | reduced loss and gradient (train.hip)
    DevBuf<char> d_dense;          // dense eigen-cuts (dense.hip): V^T, sorted vectors, eigenvalues, n_rows; allocated by the first call
    void *diverse = nullptr;       // diverse selection (diverse.hip: DiverseWs): pool rows, pair bits, accepted head; allocated by the first call
    void *multi = nullptr;         // multi-cut rounds (multirows.hip: MultiWs): head, host arrays; allocated by the first call
    void *pool = nullptr;          // cut pool (pool.hip: PoolWs): the rows of a loop, in the LP or parked; sdpcut_pool_create
    // sdpcut_shard_finish_enqueue -> sdpcut_shard_finish_wait
    int64_t shard_pending_serial = 0, shard_pending_sel = 0;
    int32_t shard_pending_world = 0, shard_pending_ld = 0;
};

// every host wait on the handle's stream goes through here: it also tells sdpcut_set_point that the
// staging copy of the previous LP point has left the host
static inline hipError_t sdpcut_sync(sdpcut_ctx *h)
{
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) h->point_inflight = false;
    return e;
}

// SDPCUT_OPT_INJECT_GIVEUP: called by the launcher of every launch that holds a bounded wait of `site` -- topk_run of topk.hip (1), the
// launchers of the CSR assemblies in rows.hip and multirows.hip (2); eligible = the launch has a wait to give up (an assembly of two workgroups at least).
// -> true: this launch is to be hit (counted; the option disarms itself with the last one).  Disarmed: one compare.
static inline bool inject_take(sdpcut_ctx *h, int site, bool eligible = true)
{
    if (h->inject_site != site || !eligible) return false;
    if (h->inject_skip > 0) { --h->inject_skip; return false; }
    if (--h->inject_count <= 0) h->inject_site = 0;
    ++h->stat_injected;
    return true;
}

// The batched calls (points.hip, tri_points.hip) leave the handle without a current point, whichever way they return: the
// single-point arrays hold, at best, the scores of the last point the per-point fallback served.
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
// The boxed batched calls leave the handle without a box, whichever way they return (the loop route and a redone point set one).
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

int sdpcut_fail(sdpcut_ctx *h, int code, const std::string &msg);
int ensure_stage(sdpcut_ctx *h, size_t bytes);   // capi.hip: grow h->d_stage
// inputs.hip: (re)allocate the device arrays of a list of N candidates, cnt[k] of them of size k
int alloc_candidates(sdpcut_ctx *h, int64_t N, const int64_t cnt[SDPCUT_MAX_K + 1], int64_t global_base);
int ensure_pinned(sdpcut_ctx *h, size_t bytes);  // capi.hip: grow h->pinned / h->pinned_dev
void free_candidates(sdpcut_ctx *h);             // inputs.hip: drop the handle's list (N = 0, nothing scored)

// the measures a strategy's selection reads (the partial strategies of a sharded round read both)
static inline uint32_t strat_need(int strat)
{
    return strat == SDPCUT_STRAT_FEAS ? SDPCUT_EIG : strat == SDPCUT_STRAT_OPT ? SDPCUT_NN : (SDPCUT_EIG | SDPCUT_NN);
}
// The selection of a skipped launch has been enqueued: from here on d_obj counts as not scored (sdpcut_ctx::obj_partial).  The
// guard does it on every way out of the scope that enqueues the selection, the refused ones included.
static inline void obj_demote(sdpcut_ctx *h)
{
    h->scored &= ~(uint32_t)SDPCUT_NN;
    h->obj_partial = true;
}
struct ObjDemoteGuard {
    sdpcut_ctx *h;
    bool on;
    ~ObjDemoteGuard() { if (on) obj_demote(h); }
};
// batch.hip: complete d_obj if it is partial (the NN-only scoring of the list: per candidate the bits the skipped launch gives)
int obj_complete(sdpcut_ctx *h);
static inline int check_round_strategy(sdpcut_ctx *h, int strat)
{
    if (strat != SDPCUT_STRAT_FEAS && strat != SDPCUT_STRAT_OPT && strat != SDPCUT_STRAT_COMB)
        return sdpcut_fail(h, SDPCUT_EINVAL, "strategy must be 1 (feasibility), 2 (optimality) or 4 (combined)");
    return 0;
}

// The pointers, n_rows and nnz of *out for a CSR round block (round_layout.h: csr_layout) of out->cap > 0 entries with rows of
// out->row_ld that lies at `block`; cap, row_ld and n_out are set already.
static inline void csr_out_from_block(const void *block, sdpcut_round_csr_t *out)
{
    const CsrLayout y = csr_layout(out->cap, out->row_ld);
    const char *b = (const char *)block;
    const int64_t *hdr = (const int64_t *)b;
    out->idx = (const int64_t *)(b + y.idx);
    out->score = (const double *)(b + y.score);
    out->lam_min = (const double *)(b + y.lam);
    out->ks = (const int32_t *)(b + y.ks);
    out->set_inds = (const int32_t *)(b + y.sets);
    out->n_rows = out->n_out > 0 ? hdr[8] : 0;
    out->nnz = out->n_out > 0 ? hdr[9] : 0;
    out->row_entry = (const int32_t *)(b + y.row_entry);
    out->indptr = (const int32_t *)(b + y.indptr);
    out->indices = (const int32_t *)(b + y.indices);
    out->values = (const double *)(b + y.values);
    out->rhs = (const double *)(b + y.rhs);
}

#define HIP_TRY(h, expr)                                                                   \
    do {                                                                                   \
        hipError_t e__ = (expr);                                                           \
        if (e__ != hipSuccess)                                                             \
            return sdpcut_fail((h), SDPCUT_EHIP,                                           \
                               std::string(#expr) + ": " + hipGetErrorString(e__));        \
    } while (0)

// The one way a buffer of the handle grows (B: DevBuf<T> or HostBuf, count in its units).  Large enough: nothing is touched.
// Else the handle's stream is waited for -- whatever was launched may still read the old block, also behind an error return that
// skipped its call's own wait -- and the buffer is reallocated: its contents are gone, *grew tells who has to fill it again.
template <class B> static inline int grow(sdpcut_ctx *h, B &buf, size_t count, bool *grew = nullptr)
{
    if (buf.size() >= count) return 0;
    HIP_TRY(h, sdpcut_sync(h));
    HIP_TRY(h, buf.reset(count));
    if (grew) *grew = true;
    return 0;
}

// The intake of a batch of LP points (n_points, points, point_ld[, lb, ub]), shared by the seven calls that take one; `prefix`
// goes in front of the texts (only sdpcut_node_eval_points has one).
static inline int check_point_batch(sdpcut_ctx *h, const char *prefix, int32_t n_points, const double *points, int64_t point_ld, int64_t min_ld)
{
    const std::string pre(prefix);
    if (n_points < 1 || n_points > SDPCUT_BATCH_MAX_POINTS)
        return sdpcut_fail(h, SDPCUT_EINVAL, pre + "n_points must be 1 .. SDPCUT_BATCH_MAX_POINTS (" + std::to_string(SDPCUT_BATCH_MAX_POINTS) + ")");
    if (!points) return sdpcut_fail(h, SDPCUT_EINVAL, pre + "points is NULL");
    if (point_ld < min_ld) return sdpcut_fail(h, SDPCUT_EINVAL, pre + "point_ld must be at least L + n");
    return 0;
}
static inline int check_box_pair(sdpcut_ctx *h, const char *prefix, const double *lb, const double *ub)
{
    if ((lb == nullptr) != (ub == nullptr)) return sdpcut_fail(h, SDPCUT_EINVAL, std::string(prefix) + "lb and ub must both be given or both be NULL");
    return 0;
}
// rows of m doubles, packed, from P rows of stride point_ld
static inline void pack_points(double *dst, int P, const double *points, int64_t point_ld, int64_t m)
{
    for (int p = 0; p < P; ++p) memcpy(dst + (size_t)p * (size_t)m, points + (size_t)p * (size_t)point_ld, (size_t)m * 8);
}
// the (l | d = u - l) rows of P boxes as sdpcut_set_box forms them, [P][2 nv] packed
static inline void pack_box_ld(double *dst, int P, int64_t nv, const double *lb, int64_t lb_ld, const double *ub, int64_t ub_ld)
{
    for (int p = 0; p < P; ++p) {
        const double *l = lb + (size_t)p * (size_t)lb_ld, *u = ub + (size_t)p * (size_t)ub_ld;
        double *d = dst + (size_t)p * 2 * (size_t)nv;
        for (int64_t i = 0; i < nv; ++i) { d[i] = l[i]; d[nv + i] = u[i] - l[i]; }
    }
}

// score.hip
// Optional: the score kernels count their scores by the leading radix digit of the selection keys
// (ScoreArgs::tk): ws = zeroed TopkWs of the selection that follows (topk_begin).
struct ScoreFuse {
    void *ws;
    int mode;      // TK_MODE_FEAS / OPT / STRONG of topk_route.h: whose keys to count
    int64_t k;     // head size of the selection (the streaming prefilter's bound rises to the k-th largest key); 0: no fine histogram
    bool emit = false;   // a skipping launch appends its strong members to the handle's emitted list (sdpcut_ctx::emit_cap)
};
// strong_out (optional, device, 8 int64 replicas): the launches add the number of candidates with
// obj_improve > 0 and lambda_min < -1e-15 to strong_out[workgroup % 8] (needs both flags; used by the device-resolved combined selection)
int launch_score(sdpcut_ctx *h, uint32_t flags, const ScoreFuse *fuse = nullptr, bool *fused = nullptr,
                 int64_t *strong_out = nullptr);
int launch_filter_audit(sdpcut_ctx *h, double *d_y32, double *d_m);   // score.hip: sdpcut_filter_audit's kernel over the (single) class 3, enqueued
int launch_cut_rows(sdpcut_ctx *h, int64_t count, const int64_t *d_limit, const int64_t *d_idx, int64_t idx_base,
                    double *d_lam, double *d_coef, int coef_ld, double *d_rhs, int64_t *d_cols, int32_t *d_ks);
// Epilogue of a fused round: rows of the ranking head + its ids, scores and the four counters,
// written to `block` (device view of the pinned host block; layout of sdpcut_select_round_view).
int launch_round_rows(sdpcut_ctx *h, int64_t cap, const int64_t *d_c4, const int64_t *d_idx, const double *d_score,
                      int coef_ld, void *block, int64_t hdr_bytes = 64, int64_t done_serial = 0);
int launch_point_copy(sdpcut_ctx *h, const double *src_mapped, int64_t n);
// rows.hip: the round's epilogue in CSR form (sdpcut_round_csr; block layout: round_layout.h, csr_layout)
int launch_round_csr(sdpcut_ctx *h, int64_t cap, const int64_t *d_c4, int64_t limit, const int64_t *d_idx, const double *d_score,
                     int ld, void *block, int64_t serial);
// rows.hip: h->d_done_ticket = the completion ticket of an epilogue launch (rows_dev.h: publish_round_done) followed by one
// look-back word per workgroup of the largest assembly grid, the multi-cut round's 512 workgroups (rows_dev.h: csr_lookback)
#define ROUND_TICKET_BYTES 64
#define ROUND_AGG_WORDS 512
int ensure_round_sync(sdpcut_ctx *h);
static inline uint64_t *round_agg_words(sdpcut_ctx *h) { return (uint64_t *)((char *)h->d_done_ticket.get() + ROUND_TICKET_BYTES); }
// eig.hip: lambda_min of every candidate, one launch over all size classes; tk = TopkWs of a feasibility selection or NULL
int launch_eig_only(sdpcut_ctx *h, void *tk, hipEvent_t ev_start, hipEvent_t ev_stop, int64_t pf_k = 0);
// the point-axis forms of the scoring and of the CSR assembly (a batch of LP points, points.hip): eig.hip, score.hip, rows.hip
int launch_eig_only_points(sdpcut_ctx *h, int n_points, const double *d_pts, int64_t pts_stride, double *d_eig, int64_t eig_stride);
bool score_points_served(const sdpcut_ctx *h, uint32_t flags);
int launch_score_points(sdpcut_ctx *h, uint32_t flags, int n_points, const double *d_pts, int64_t pts_stride, double *d_eig, double *d_obj,
                        int64_t score_stride, int64_t *d_strong, int64_t strong_stride, const double *d_Q = nullptr, int64_t Q_stride = 0);
int launch_round_csr_points(sdpcut_ctx *h, int p_first, int n_points, int64_t cap, int ld, const int64_t *d_c4, int64_t c4_stride,
                            const int64_t *d_idx, const double *d_score, const double *d_pts, int64_t pts_stride, const double *d_eig,
                            int64_t eig_stride, uint64_t *d_agg, int64_t agg_stride, void *block, int64_t block_stride, int64_t serial);
int wait_round_done(sdpcut_ctx *h, const int64_t *word, int64_t serial);   // round.hip
// round.hip: a CSR assembly into the handle's pinned block, launched here and waited for, once more if its look-back gave up
int csr_assemble_wait(sdpcut_ctx *h, int last_word, int launches, bool count_failure, const char *what,
                      const std::function<int(int64_t serial)> &launch);
int score_for_selection(sdpcut_ctx *h, int strat, int64_t sel_size, int64_t cap, uint32_t need, bool allow_auto, int *stage,
                        bool *auto_out);                                   // round.hip
// batch_kernels.hip
int launch_eig_batch(sdpcut_ctx *h, int k, int64_t count, const double *d_x, const double *d_X,
                     double *d_vals, double *d_vecs);
int launch_nn_batch(sdpcut_ctx *h, int k, int64_t count, const double *d_in, double *d_out);
int launch_mfma_probe(sdpcut_ctx *h, const double *d_A, const double *d_B, double *d_C);

// rank.hip
int ensure_rank_ws(sdpcut_ctx *h, int64_t n);
int ensure_key_ws(sdpcut_ctx *h, int64_t n);
int rank_on_device(sdpcut_ctx *h, int strat, int64_t sel_size, int64_t max_out, int64_t *d_idx_out,
                   double *d_score_out, int64_t *n_written, int64_t *n_total, int32_t *new_strat,
                   int64_t *counters, int64_t strong_hint = -1);
int merge_topk_on_device(sdpcut_ctx *h, int64_t count, const double *d_scores, const double *d_secondary,
                         const int64_t *d_ids, int64_t max_out, double *d_score_out, int64_t *d_id_out);
int gather_scores_on_device(sdpcut_ctx *h, int64_t count, const int64_t *d_ids, double *d_eig_out, double *d_obj_out);
int rank_fetch_on_device(sdpcut_ctx *h, int64_t offset, int64_t count, int64_t *d_idx_out, double *d_score_out);

// stage: see topk_select_enqueue; auto_regime: the combined strategy's regime is resolved on the device
// from the strong count the score kernels of this round left in the selection workspace
int rank_fast_enqueue(sdpcut_ctx *h, int strat, int64_t sel_size, int64_t max_out, int64_t *d_idx_out,
                      double *d_score_out, const int64_t **d_c4, int stage = 0, bool auto_regime = false);
// TK_MODE_* the fast path would use for this request, 0 if it is not eligible
int rank_fast_mode(sdpcut_ctx *h, int strat, int64_t sel_size, int64_t max_out, double *score_add);
int rank_fast_finish(sdpcut_ctx *h, int strat, int64_t sel_size, int64_t max_out, const int64_t c4[7],
                     int64_t *n_written, int64_t *n_total, int32_t *new_strat, int64_t *counters_out);

// exact_head.hip (SDPCUT_OPT_EXACT_HEAD)
int exact_head_applies(const sdpcut_ctx *h, int strat);      // option on, strategy 2 or 4
int64_t exact_first_band(const sdpcut_ctx *h, int64_t cap);  // entries of the first band of a head of cap entries
int64_t exact_widest_band(const sdpcut_ctx *h);
int exact_head_enqueue(sdpcut_ctx *h, int strat, int64_t sel_size, int64_t cap, int64_t band, int64_t *d_idx_out, double *d_score_out,
                       const int64_t **d_c4);
int exact_head_verdict(sdpcut_ctx *h, const int64_t c4[7], int64_t band);   // 0 exact, 1 retry with the widest band, 2 give up
// the sharded entry points have no exact merge
#define SDPCUT_NO_EXACT(h)                                                                                                \
    do {                                                                                                                  \
        if ((h)->exact_head)                                                                                              \
            return sdpcut_fail((h), SDPCUT_ESTATE, "SDPCUT_OPT_EXACT_HEAD is on: the sharded rounds have no exact merge"); \
    } while (0)

// box.hip (node boxes, include/sdpcut.h: sdpcut_set_box)
// the tables a launch that computes `flags` reads: the box tables where a box is set and the launch computes SDPCUT_NN or SDPCUT_SDP
// (never together with SDPCUT_EIG: launch_score splits such a call), else the originals
static inline const double *score_vars(const sdpcut_ctx *h, uint32_t flags)
{
    return (h->box_set && (flags & (SDPCUT_NN | SDPCUT_SDP)) && !(flags & SDPCUT_EIG)) ? h->d_vars_box.get() : h->d_vars.get();
}
static inline const double *score_Q(const sdpcut_ctx *h, uint32_t flags)
{
    return (h->box_set && (flags & (SDPCUT_NN | SDPCUT_SDP)) && !(flags & SDPCUT_EIG)) ? h->d_Q_box.get() : h->d_Q.get();
}
int box_after_point(sdpcut_ctx *h);   // the transformed point from d_vars, behind its copy on the handle's stream; nothing without a box
void box_clear(sdpcut_ctx *h);        // drop the box and its tables (the caller has waited for the stream)
// sdpcut_set_box's rule on one box, the failure recorded in the name of `what` (point >= 0: "point <point>, variable <i>")
int box_check(sdpcut_ctx *h, const char *what, int point, const double *lb, const double *ub);
// box_points_kernel: Q' (rows of L) and the transformed points (rows of L + n) of n_points points, each in the box of its row of
// the [n_points][2 n] (l | d) table d_ld; d_Qb NULL: the transformed points alone
int launch_box_points(sdpcut_ctx *h, int n_points, const double *d_pts, int64_t pts_stride, const double *d_ld, double *d_Qb, double *d_vb);
#define SDPCUT_NO_BOX(h, what)                                                                                            \
    do {                                                                                                                  \
        if ((h)->box_set)                                                                                                 \
            return sdpcut_fail((h), SDPCUT_ESTATE, std::string(what) + ": a node box is set (sdpcut_set_box); clear it first"); \
    } while (0)

// diverse.hip
void free_diverse_ws(sdpcut_ctx *h);
// The filter of a batch of points (div_rows_points_kernel, div_points_kernel): point p reads the head its selection emitted (row p
// of idx / score, `pool` entries per row, its length and void flag in sel_c4 + p * c4_stride) and its LP point, and writes the
// accepted entries into row p of acc_idx / acc_score (`cap` entries per row), the walk's counts into info + 8 p, and the
// selection's counters into sel_out + 8 p (host memory).  row_*: scratch for the pool's rows, [n_points][pool].
#define DIVP_MAX_POOL 512      // = BATCH_DIVERSE_MAX_POOL of batch_route.h: the rows of a pool fit the LDS of one workgroup
#define DIVP_THREADS 512
struct DivPointsArgs {
    int64_t pool, cap, quota;
    double max_parallel;
    int compare;               // max_parallel < 1
    const int64_t *sel_c4;
    int64_t c4_stride;
    const int64_t *idx;
    const double *score;
    int64_t idx_base, n_local;
    const int32_t *set5, *ks;
    const double *vars;
    int64_t vars_ld;
    int32_t nv;
    int64_t L;
    const double *eig;         // [n_points][eig_ld] lambda_min where the scoring computed it, else NULL
    int64_t eig_ld;
    double *row_coef, *row_lam;
    int32_t *row_ks;
    int64_t *acc_idx;
    double *acc_score;
    int64_t *info, *sel_out;
};
int launch_div_points(sdpcut_ctx *h, int n_points, const DivPointsArgs &A);
// multirows.hip
void free_multi_ws(sdpcut_ctx *h);
// pool.hip
void free_pool_ws(sdpcut_ctx *h);

// exact_sdp.hip (SDPCUT_SDP, SDPCUT_OPT_EXACT_SDP)
int launch_exact_sdp(sdpcut_ctx *h);                 // d_sdp / d_sdp_gap of every candidate at the current point
int sdp_unconverged(sdpcut_ctx *h, int64_t *value);  // SDPCUT_STAT_SDP_UNCONVERGED (waits for the handle's stream)
void free_sdp_ws(sdpcut_ctx *h);
// Strategies 3 and 6 = strategy 2 on another measure (3: the exact measure of SDPCUT_SDP, cut_select_qp.py:584-601 -- the same list,
// the same sort, another obj_improve; 6: the efficacy score of SDPCUT_EFF).  The non-fused selection reads the handle's optimality
// array wherever it ranks (rank.hip, topk.hip); for the lifetime of this object that array IS the measure's (d_sdp / d_escore) and
// its `scored` bit is the measure's, and SDPCUT_OPT_EXACT_HEAD -- which re-scores the MLP -- is off.  Nothing scores inside a view:
// its scope begins after the measure has been scored.  The measure is whole whatever a skipped round left of the MLP's
// (obj_partial): inside the view that flag is down -- obj_complete has nothing to do there and must not, its launch would write the
// MLP's scores into the measure's array -- and the real array's state comes back with the array.
struct MeasureAsObj {
    sdpcut_ctx *h;
    double *obj;
    uint32_t scored;
    bool exact_head, obj_partial;
    MeasureAsObj(sdpcut_ctx *ctx, uint32_t measure)
        : h(ctx), obj(ctx->d_obj), scored(ctx->scored), exact_head(ctx->exact_head), obj_partial(ctx->obj_partial)
    {
        h->d_obj = measure == SDPCUT_EFF ? h->d_escore : h->d_sdp.get();
        h->scored = (scored & SDPCUT_EIG) | ((scored & measure) ? (uint32_t)SDPCUT_NN : 0u);
        h->exact_head = false;
        h->obj_partial = false;
    }
    ~MeasureAsObj()
    {
        h->d_obj = obj;
        h->scored = scored;
        h->exact_head = exact_head;
        h->obj_partial = obj_partial;
    }
    MeasureAsObj(const MeasureAsObj &) = delete;
    MeasureAsObj &operator=(const MeasureAsObj &) = delete;
};
// the measure a strategy ranks by through such a view, 0 for the strategies with a selection of their own: strategy 3 where it is
// accepted (the option on, else the caller's own refusal of an unknown strategy stands) and strategy 6
static inline uint32_t strat_view(const sdpcut_ctx *h, int strat)
{
    return (strat == SDPCUT_STRAT_EXACT && h->exact_sdp) ? (uint32_t)SDPCUT_SDP : strat == SDPCUT_STRAT_EFF ? (uint32_t)SDPCUT_EFF : 0u;
}
static inline int view_strat(uint32_t measure) { return measure == SDPCUT_EFF ? SDPCUT_STRAT_EFF : SDPCUT_STRAT_EXACT; }

// efficacy.hip (SDPCUT_EFF)
int launch_efficacy(sdpcut_ctx *h);                  // d_eff / d_objpar / d_escore of every candidate at the current point; needs d_eig
int launch_efficacy_points(sdpcut_ctx *h, int n_points, const double *d_pts, int64_t pts_stride, const double *d_eig, int64_t score_stride,
                           double *d_eff, double *d_objpar, double *d_escore);   // the same at every point of a batch
void free_eff_ws(sdpcut_ctx *h);
void free_lpobj(sdpcut_ctx *h);

// tri.hip
int tri_preprocess(sdpcut_ctx *h, const uint8_t *adjacency, int64_t *n_triples);
int tri_separate(sdpcut_ctx *h, int64_t max_out, int64_t *d_entry_out, double *d_viol_out, int64_t *n_violated,
                 int64_t *n_written);
// the pointers and counts of *out for a triangle block (tri_layout.h: tri_layout) of out->cap entries that lies at `block`
void tri_out_from_block(const void *block, sdpcut_tri_csr_t *out);
// tri_points.hip
void free_tri_points_ws(sdpcut_ctx *h);
void free_node_eval_ws(sdpcut_ctx *h);               // node_eval.hip

// topk.hip
int topk_select_enqueue(sdpcut_ctx *h, int mode, int64_t k, double score_add, int64_t *d_idx_out,
                        double *d_score_out, const int64_t **d_counters_out, int stage = 0, int64_t sel = 0);
// allocate / zero (or swap in the pre-zeroed) workspace of the next selection and return it together
// with the key array: what a score launch needs to run the selection's first pass itself
// (ScoreFuse); follow with topk_select_enqueue(..., stage = 3)
int topk_begin(sdpcut_ctx *h, void **ws, uint64_t **keys);
bool topk_fuse_ok(const sdpcut_ctx *h, int64_t k, bool comb);     // may a score launch take a ScoreFuse for a head of k entries?
int64_t *topk_strong_counter(void *ws);      // TopkWs::strong_rep (TK_SREP = 8 replicas) of a workspace handed out by topk_begin
int topk_select_on_device(sdpcut_ctx *h, int mode, int64_t k, double score_add, int64_t *d_idx_out,
                          double *d_score_out, int64_t cnt[5]);
int topk_select_keys_on_device(sdpcut_ctx *h, int64_t n, int64_t k, int64_t *d_idx_out, double *d_val_out, int64_t cnt[5]);
// the same selection enqueued, without the host wait: *d_counters_out = its five counters on the device (what `cnt` receives)
int topk_select_keys_enqueue(sdpcut_ctx *h, int64_t n, int64_t k, int64_t *d_idx_out, double *d_val_out, const int64_t **d_counters_out);
// the void COMBALL selection in the handle's workspace, answered by two selections over precomputed keys (see topk.hip)
int topk_tie_split(sdpcut_ctx *h, int64_t k, int64_t *d_idx_out, double *d_score_out, int64_t *k_eff_out);
// the workspace NOT used by the selection enqueued last, and its size in 8-byte words: a later
// kernel of the same stream may zero it and then set h->topk_alt_clean (saves the next memset)
int topk_alt_ws(sdpcut_ctx *h, uint64_t **ptr, int *words);
