// Scoring of the handle's candidate list, host side: launch_score decides the form of the call (score_form, score_plan.h) and
// drives the launches -- the eigenvalue-only kernel (eig.hip), one launch over all size classes, the classes side by side on side
// streams or one after the other.  The kernels and the launchers that start them are in score_mfma.hip and score_alt.hip
// (score_launch.h); no kernel is defined or referenced here.
#include "score_launch.h"

// does size class K run on the MFMA / VALU kernels (network shape they are instantiated for)?
static bool net_shape_ok(const sdpcut_ctx *h, int K, uint32_t flags)
{
    if (!(flags & SDPCUT_NN)) return true;   // eig only: the network part of the kernel is skipped
    return h->net[K].set && net_shape_is(K, h->net[K].dev.width, h->net[K].dev.n_hidden);
}

static ScorePlan plan_class(const sdpcut_ctx *h, int K, const ScoreFuse *fuse)
{
    return score_plan(h->bucket[K].n, h->n_cu, K, h->N, fuse ? fuse->k : 0, fuse != nullptr);
}

// one launch over size class K (nothing if it is empty); score_form has accepted the call
static int launch_score_k(sdpcut_ctx *h, int K, uint32_t flags, hipEvent_t ev_start, hipEvent_t ev_stop, const ScoreFuse *fuse,
                          int64_t *strong_out, hipStream_t st = nullptr)
{
    if (h->bucket[K].n == 0) return 0;
    if (!st) st = h->stream;
    const bool shaped = net_shape_ok(h, K, flags);
    // SDPCUT_OPT_SKIP_NONVIOLATED: the fused launch of a combined round (the strong class is all it counts for) over a list of
    // this one class runs the MLP for violated candidates only; d_obj is then valid for those alone (obj_demote)
    const bool skip = fuse && fuse->mode == TK_MODE_STRONG && flags == (uint32_t)(SDPCUT_EIG | SDPCUT_NN) && shaped &&
                      h->kernel_variant == SDPCUT_KERNEL_MFMA && h->bucket[K].n == h->N && score_mfma_skip_built(K) &&
                      score_skip_applies(h->bucket[K].n, h->n_cu, K, h->skip_nonviolated);
    const ScorePlan p = skip ? score_plan_skip(h->bucket[K].n, h->n_cu, K, h->N, fuse->k, h->skip_nonviolated == 2) : plan_class(h, K, fuse);
    ScoreArgs A = fill_score_args(h, K, flags, fuse, strong_out, p);
    if (skip) {
        if (A.pf_mloc == 0) h->pf_counted = false;
        // SDPCUT_OPT_EMIT_HEAD: the strong members go to a list in the key array, which a selection that starts from this launch's
        // histograms (stage 3) does not use: 16 bytes per entry, the key and the index
        int64_t ecap = fuse->emit && A.strong_out && h->d_key_a.get() ? (int64_t)h->d_key_a.size() / 2 : 0;
        if (ecap > 0xffffffffll) ecap = 0xffffffffll;
        if (h->emit_cap_opt > 0 && h->emit_cap_opt < ecap) ecap = h->emit_cap_opt;
        if (ecap > 0) {
            A.emit = h->d_key_a.get();
            A.emit_cap = (uint32_t)ecap;
            h->emit_launched = true;
            h->emit_cap = ecap;
        }
        // SDPCUT_OPT_FP32_FILTER: an fp32 pass with a proven error bound in front of the fp64 one (NetDev::filter_ok)
        const bool filter = h->fp32_filter && A.net.filter_ok && score_mfma_filter_built(K);
        if (filter) score_mfma_filter_launch(K, A, p.grid, st, ev_start, ev_stop);
        else score_mfma_skip_launch(K, A, p.grid, st, ev_start, ev_stop);
        h->skip_launched = true;
        h->filter_launched = filter;
    } else if (h->kernel_variant == SDPCUT_KERNEL_MFMA && shaped) {
        if (A.tk && A.pf_mloc == 0) h->pf_counted = false;
        score_mfma_launch(K, A, p.grid, st, ev_start, ev_stop);
    } else
        score_alt_launch(K, h->kernel_variant == SDPCUT_KERNEL_VALU && shaped, A, h->n_cu, st, ev_start, ev_stop);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// One launch over all size classes of the list (score_mfma_all_kernel; when it applies: SCORE_FORM_ONE of score_form).  Every
// class gets the plan -- and so the scores -- of a launch over this class alone.
static int launch_classes_one(sdpcut_ctx *h, uint32_t flags, const ScoreFuse *fuse, int64_t *strong_out, hipEvent_t ev_start,
                              hipEvent_t ev_stop)
{
    ScoreArgsAll AA;
    int order[SDPCUT_MAX_K - 1], m = 0;
    for (int k = 2; k <= SDPCUT_MAX_K; ++k)
        if (h->bucket[k].n > 0) order[m++] = k;
    for (int i = 1; i < m; ++i)      // the largest class first: its workgroups are the launch's critical path
        for (int j = i; j > 0 && h->bucket[order[j]].n > h->bucket[order[j - 1]].n; --j) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
    int64_t blocks = 0;
    for (int i = 0; i < m; ++i) {
        const int k = order[i];
        const ScorePlan p = plan_class(h, k, fuse);
        AA.a[i] = fill_score_args(h, k, flags, fuse, strong_out, p);
        if (AA.a[i].tk && p.pf_mloc == 0) h->pf_counted = false;
        blocks += p.grid;
        AA.k[i] = k;
        AA.bend[i] = (int32_t)blocks;
    }
    AA.nclasses = m;
    score_mfma_all_launch(AA, h->stream, ev_start, ev_stop);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

static int ensure_side_streams(sdpcut_ctx *h)
{
    if (h->ev_fork) return 0;
    // at the device's highest priority: the runtime keeps separate hardware queues per priority level, so the side streams do not
    // land in the queue of the handle's own (normal-priority) stream however many streams the process has created before -- in
    // a process that also runs torch they did, and the classes ran one after the other again, plus the events -- and their few
    // workgroups are dispatched ahead of the large class's waiting ones
    int least = 0, greatest = 0;
    HIP_TRY(h, hipDeviceGetStreamPriorityRange(&least, &greatest));
    for (int i = 0; i < 3; ++i) {
        HIP_TRY(h, hipStreamCreateWithPriority(&h->side_stream[i], hipStreamNonBlocking, greatest));
        HIP_TRY(h, hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming));
    }
    HIP_TRY(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    return 0;
}

// the size classes one launch after the other on the handle's stream
static int launch_classes_seq(sdpcut_ctx *h, uint32_t flags, const ScoreFuse *fuse, int64_t *strong_out, const hipEvent_t *es,
                              const hipEvent_t *ee)
{
    for (int k = 2; k <= SDPCUT_MAX_K; ++k) {
        const int rc = launch_score_k(h, k, flags, es ? es[k] : nullptr, ee ? ee[k] : nullptr, fuse, strong_out, nullptr);
        if (rc) return rc;
    }
    return 0;
}

// Several size classes: real covers hold one large class and a few sets of the smaller sizes (spar100-050-1, dim 5: 72 673
// five-variable sets, 103 of four, 1 of three), and a launch over a hundred candidates costs what one pass costs -- 25-55 us of
// dependent stages -- however few they are.  Here the small classes go to side streams between a fork and a join event, the
// largest first on the handle's stream (its launch is what the round waits for).  Scores land in disjoint slots, the
// histograms are atomics: no order is needed.
static int launch_classes_side(sdpcut_ctx *h, uint32_t flags, const ScoreFuse *fuse, int64_t *strong_out, int kbig)
{
    int rc = ensure_side_streams(h);
    if (rc) return rc;
    HIP_TRY(h, hipEventRecord(h->ev_fork, h->stream));
    if ((rc = launch_score_k(h, kbig, flags, nullptr, nullptr, fuse, strong_out, nullptr))) return rc;
    int side = 0;
    for (int k = 2; k <= SDPCUT_MAX_K; ++k) {
        if (k == kbig || h->bucket[k].n == 0) continue;
        hipStream_t st = h->side_stream[side];
        HIP_TRY(h, hipStreamWaitEvent(st, h->ev_fork, 0));
        if ((rc = launch_score_k(h, k, flags, nullptr, nullptr, fuse, strong_out, st))) return rc;
        HIP_TRY(h, hipEventRecord(h->ev_join[side], st));
        ++side;
    }
    for (int i = 0; i < side; ++i) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_join[i], 0));
    return 0;
}

// Whether the side streams pay is a property of the process, not of the list: streams share a few hardware queues, assigned as
// they are created, and a side stream that lands in the queue of the handle's own stream runs its class BEHIND the large one --
// 193 instead of 154 us per round on spar070-050-1 in one process, 141 in another (profiles/r03_mixed_cover_round_timeline.txt).
// So the first multi-class scoring of a candidate list measures both forms (three plain scoring passes each, no histograms,
// the same scores written six times: ~1 ms once per list) and keeps the faster.
static int calibrate_side_streams(sdpcut_ctx *h, uint32_t flags, int kbig)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(h, hipEventCreate(&e0));
    HIP_TRY(h, hipEventCreate(&e1));
    float best[2] = {1e30f, 1e30f};
    int rc = 0;
    for (int rep = 0; rep < 3 && !rc; ++rep)
        for (int form = 0; form < 2 && !rc; ++form) {
            (void)hipEventRecord(e0, h->stream);
            rc = form ? launch_classes_side(h, flags, nullptr, nullptr, kbig) : launch_classes_seq(h, flags, nullptr, nullptr, nullptr, nullptr);
            (void)hipEventRecord(e1, h->stream);
            if (!rc && hipEventSynchronize(e1) != hipSuccess) rc = sdpcut_fail(h, SDPCUT_EHIP, "side-stream calibration failed");
            float ms = 0.f;
            if (!rc && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms < best[form]) best[form] = ms;
        }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    h->side_choice = best[1] < 0.97f * best[0] ? 1 : 0;
    h->side_ms[0] = best[0];
    h->side_ms[1] = best[1];
    return 0;
}

// what score_form is asked about a call on this handle
static ScoreFormIn form_in(const sdpcut_ctx *h, uint32_t flags, const ScoreFuse *fuse)
{
    ScoreFormIn in;
    in.variant = h->kernel_variant;
    in.flags = flags;
    for (int k = 2; k <= SDPCUT_MAX_K; ++k) {
        const NetHost &net = h->net[k];
        in.n[k] = h->bucket[k].n;
        in.net_set[k] = net.set;
        in.shape_ok[k] = net.set && net_shape_is(k, net.dev.width, net.dev.n_hidden);
        in.unclamped_ok[k] = net.set && net.dev.unclamped_ok;
    }
    in.n_total = h->N;
    in.fuse = fuse != nullptr;
    in.fuse_mode = fuse ? fuse->mode : 0;
    in.eig_kernel = h->eig_kernel;
    in.one_launch = h->one_launch;
    in.side_streams = h->side_streams;
    in.side_choice = h->side_choice;
    in.timing = h->timing;
    return in;
}

static int launch_score_form(sdpcut_ctx *h, uint32_t flags, const ScoreFuse *fuse, bool *fused, int64_t *strong_out)
{
    // (r5) did EVERY launch of this round count the fine histogram of the selection's class?  (The selection reads the table only then.)
    h->pf_counted = fuse != nullptr && fuse->k > 0;
    h->skip_launched = false;      // set by the launch that skips (launch_score_k)
    h->emit_launched = false;      // ... and emits
    h->filter_launched = false;
    const ScoreFormIn in = form_in(h, flags, fuse);
    const ScoreForm f = score_form(in);
    if (fused) *fused = f.fused;
    if (f.err) return sdpcut_fail(h, f.err, score_form_msg(f.msg));
    if (!f.fused) fuse = nullptr;
    h->timed_score = f.timed;
    hipEvent_t ev_start = f.timed ? h->ev[0] : nullptr, ev_stop = f.timed ? h->ev[1] : nullptr;
    if (f.form == SCORE_FORM_EIG)      // a pure-feasibility scan has its own kernel: one launch over all size classes (eig.hip)
        return launch_eig_only(h, fuse ? fuse->ws : nullptr, ev_start, ev_stop, fuse ? fuse->k : 0);
    if (f.form == SCORE_FORM_ONE) return launch_classes_one(h, flags, fuse, strong_out, ev_start, ev_stop);
    bool side = f.form == SCORE_FORM_SIDE;
    if (f.calibrate) {
        const int rc = calibrate_side_streams(h, flags, f.kbig);
        if (rc) return rc;
        side = h->side_choice == 1;
    }
    if (side) return launch_classes_side(h, flags, fuse, strong_out, f.kbig);
    // the first non-empty size class carries the start event, the last one the stop event
    hipEvent_t es[SDPCUT_MAX_K + 1] = {}, ee[SDPCUT_MAX_K + 1] = {};
    es[f.first] = ev_start;
    ee[f.last] = ev_stop;
    return launch_classes_seq(h, flags, fuse, strong_out, es, ee);
}

int launch_score(sdpcut_ctx *h, uint32_t flags, const ScoreFuse *fuse, bool *fused, int64_t *strong_out)
{
    int rc;
    if (h->box_set && (flags & SDPCUT_EIG) && (flags & SDPCUT_NN)) {
        // a node box: lambda_min from the original tables, the optimality measure from the box tables -- two launches, nothing
        // counted for a selection (no class of the keys can be told from one of them alone: round.hip scores first with a box)
        if (fuse || strong_out) return sdpcut_fail(h, SDPCUT_ESTATE, "score: no fused launch while a node box is set");
        if (fused) *fused = false;
        rc = launch_score_form(h, SDPCUT_EIG, nullptr, nullptr, nullptr);
        if (!rc) rc = launch_score_form(h, SDPCUT_NN, nullptr, nullptr, nullptr);
    } else {
        rc = launch_score_form(h, flags, fuse, fused, strong_out);
    }
    // a launch that wrote the optimality measure of every candidate has completed what a skipped round left partial
    if (!rc && (flags & SDPCUT_NN) && h->obj_partial && !h->skip_launched) {
        h->obj_partial = false;
        ++h->stat_nn_completions;
    }
    if (!rc && !h->skip_launched) {      // SDPCUT_STAT_NN_SKIPPED is the LAST scoring launch's: this one skipped nobody
        h->stat_nn_skipped = 0;
        h->nn_skipped_on_device = false;
    }
    // SDPCUT_STAT_NN_EVALUATED: a launch that ran the network ran it for everybody (N), for the violated candidates (a skipping
    // launch: N - SDPCUT_STAT_NN_SKIPPED) or for the filter's survivors (counted on the device, d_stats[5])
    if (!rc && (flags & SDPCUT_NN)) {
        h->nn_eval_mode = h->filter_launched ? 2 : h->skip_launched ? 1 : 0;
        h->nn_eval_n = h->N;
    }
    return rc;
}

// ---- a batch of LP points (points.hip) ------------------------------------------------------------------------------------------
// Do the point-axis kernels serve a scoring of `flags` on this handle?  The eigenvalue-only kernel (flags == SDPCUT_EIG) and the
// MFMA kernel have one; the VALU / simple variants and networks of another shape (score_alt.hip) do not: such a batch is scored
// point by point through launch_score.  A call launch_score would refuse is "served": launch_score_points refuses it the same way.
bool score_points_served(const sdpcut_ctx *h, uint32_t flags)
{
    const ScoreFormIn in = form_in(h, flags, nullptr);
    const ScoreForm f = score_form(in);
    if (f.err || f.form == SCORE_FORM_EIG) return true;
    if (in.variant != SDPCUT_KERNEL_MFMA) return false;
    for (int k = 2; k <= SDPCUT_MAX_K; ++k)
        if (in.n[k] > 0 && !score_class_shaped(in, k)) return false;
    return true;
}

// The scores of the handle's list at n_points LP points, rows of d_pts (stride pts_stride), into rows of d_eig / d_obj (stride
// score_stride): ONE launch with a point axis for an eigenvalue-only scan, else one per size class (every class with the plan -- and
// so the scores -- of its single-point launch).  d_strong (optional, needs both flags): point p's launches add its strong
// candidates to the eight replicas at d_strong + p * strong_stride.  d_Q (optional; a boxed batch, points.hip): the MFMA launches
// read point p's instance table at d_Q + p * Q_stride instead of the handle's one Q.
int launch_score_points(sdpcut_ctx *h, uint32_t flags, int n_points, const double *d_pts, int64_t pts_stride, double *d_eig, double *d_obj,
                        int64_t score_stride, int64_t *d_strong, int64_t strong_stride, const double *d_Q, int64_t Q_stride)
{
    const ScoreFormIn in = form_in(h, flags, nullptr);
    const ScoreForm f = score_form(in);
    if (f.err) return sdpcut_fail(h, f.err, score_form_msg(f.msg));
    if (!score_points_served(h, flags)) return sdpcut_fail(h, SDPCUT_ESTATE, "score: this kernel variant has no point axis");
    if (f.form == SCORE_FORM_EIG) return launch_eig_only_points(h, n_points, d_pts, pts_stride, d_eig, score_stride);
    const ScorePointStrides ps = {pts_stride, score_stride, strong_stride, d_Q ? Q_stride : 0};
    for (int k = 2; k <= SDPCUT_MAX_K; ++k) {
        if (h->bucket[k].n == 0) continue;
        const ScorePlan p = plan_class(h, k, nullptr);
        ScoreArgs A = fill_score_args(h, k, flags, nullptr, d_strong, p);
        A.vars = d_pts; A.eig_out = d_eig; A.obj_out = d_obj;
        if (d_Q) A.Q = d_Q;
        score_mfma_points_launch(k, A, ps, p.grid, n_points, h->stream);
    }
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// sdpcut_filter_audit: the filter's fp32 pass for every candidate of a list of 3-variable candidates (the caller has checked that)
int launch_filter_audit(sdpcut_ctx *h, double *d_y32, double *d_m)
{
    const int K = 3;
    const uint32_t flags = SDPCUT_EIG | SDPCUT_NN;
    const ScorePlan p = plan_class(h, K, nullptr);
    const ScoreArgs A = fill_score_args(h, K, flags, nullptr, nullptr, p);
    const int64_t rounds = (h->bucket[K].n + 127) / 128;      // a workgroup takes 128 candidates at a time
    const int grid = (int)(rounds < 4 * (int64_t)h->n_cu ? (rounds < 1 ? 1 : rounds) : 4 * (int64_t)h->n_cu);
    score_filter_audit_launch(K, A, grid, d_y32, d_m, h->stream);
    HIP_TRY(h, hipGetLastError());
    return 0;
}
