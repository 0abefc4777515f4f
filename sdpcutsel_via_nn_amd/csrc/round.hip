// The fused round (include/sdpcut.h: sdpcut_select_round*, sdpcut_round_view, sdpcut_round_csr*): score -> rank -> rows in one
// enqueue, one host wait.
#include <cstring>

#include "common.h"
#include "topk_route.h"

// Host wait for the serial number the last workgroup of a round's epilogue stores (system scope, after
// its results) into pinned memory.  Bounded: after ~2 s without the word the stream is synchronised
// the ordinary way, which also surfaces a faulted kernel as an error.
int wait_round_done(sdpcut_ctx *h, const int64_t *word, int64_t serial)
{
    const volatile int64_t *w = (const volatile int64_t *)word;
    for (long spin = 0; spin < 400000000L; ++spin) {
        if (*w == serial) {
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            h->point_inflight = false;      // the round ran behind the point's transfer
            return 0;
        }
        __builtin_ia32_pause();
        if ((spin & 0xfffff) == 0xfffff && hipStreamQuery(h->stream) != hipErrorNotReady) break;
    }
    HIP_TRY(h, sdpcut_sync(h));
    if (*w != serial) return sdpcut_fail(h, SDPCUT_EHIP, "round epilogue did not report completion");
    return 0;
}

// Scores of a round's selection (strategy strat, head of `cap` entries), not computed yet at this point:
// *stage / *auto_out are what topk_select_enqueue / rank_fast_enqueue take.
// If nothing has been scored at the point and the head comes from the radix select, the score kernels work
// for the selection that follows.  Combined strategy (allow_auto): they count the strong candidates into
// its workspace and the selection resolves its regime on the device (at least sel_size strong ones:
// those, + BIG_M; fewer: every entry visited) -- one selection and no host round trip in either regime.
// SDPCUT_OPT_FUSE_KEYS: they also count the class members by the leading digit of the selection keys, so
// that the selection starts at its second digit and needs no key pass (the every-entry-visited regime of
// the combined strategy runs its own first digit inside the selection).
int score_for_selection(sdpcut_ctx *h, int strat, int64_t sel_size, int64_t cap, uint32_t need, bool allow_auto, int *stage,
                        bool *auto_out)
{
    *stage = 0;
    *auto_out = false;
    h->skip_launched = false;
    h->emit_launched = false;
    int rc;
    // a measure a skipped round left partial (same point, another selection): whole before anything ranks or counts by it -- a
    // feasibility selection too, whose nb_positive reads it
    if ((rc = obj_complete(h))) return rc;
    // a node box: the optimality measure comes from other tables than lambda_min, so no one launch can count for the selection --
    // score first (sdpcut_score: an EIG launch on the original tables, an NN launch on the box tables); the selection below is
    // then the one of a list scored already
    if (h->box_set && (need & SDPCUT_NN) && (h->scored & need) != need && (rc = sdpcut_score(h, need & ~h->scored))) return rc;
    const int fast_mode = (h->scored & need) == 0 ? rank_fast_mode(h, strat, sel_size, cap, nullptr) : 0;
    const bool want_auto = allow_auto && strat == SDPCUT_STRAT_COMB;
    // (the short-list predicate must be the one topk_select_enqueue will evaluate: it sees the tie-aware combined modes only when
    // the regime is resolved on the device -- a combined round whose mode the HOST resolved runs as TK_MODE_STRONG)
    const bool count_digit = h->fuse_keys && topk_fuse_ok(h, cap, want_auto);
    if (fast_mode && (want_auto || count_digit)) {
        void *ws = nullptr;
        rc = topk_begin(h, &ws, nullptr);
        if (rc) return rc;
        int64_t *strong = (need == (SDPCUT_EIG | SDPCUT_NN)) ? topk_strong_counter(ws) : nullptr;
        bool counted = false;
        if (count_digit) {
            ScoreFuse fuse;
            fuse.ws = ws;
            fuse.mode = fast_mode;
            fuse.k = (h->prefilter && h->N >= SDPCUT_PF_MIN_N) ? cap : 0;
            fuse.emit = want_auto && h->emit_head;      // only a regime resolved on the device reads the list (TK_ROUTE_EMITTED)
            rc = launch_score(h, need, &fuse, &counted, strong);
        } else {
            rc = launch_score(h, need, nullptr, nullptr, strong);
        }
        if (rc) return rc;
        h->scored |= need;
        *stage = counted ? 3 : 1;
        *auto_out = want_auto;
    } else if ((h->scored & need) != need) {
        rc = sdpcut_score(h, need & ~h->scored);
        if (rc) return rc;
    }
    return 0;
}

// One fused round in two halves: round_begin enqueues everything -- score (if needed) -> rank -> epilogue into the pinned block --
// WITHOUT waiting; round_end waits, reads the counters and, when the enqueued selection is not the answer (a void one; the
// combined scan of heads > 8192), runs the general path.  csr = false: padded rows, block layout of sdpcut_select_round_view
// (rows_layout behind 64 bytes; the staging area mirrors it); csr = true: the CSR block of sdpcut_round_csr (csr_layout).
// Two handles may both begin before either ends: their device work overlaps (the QCQP round's two covers).
static int round_begin_exact_again(sdpcut_ctx *h, PendingRound &P);
static int round_begin(sdpcut_ctx *h, int strat, int64_t sel_size, int32_t coef_ld, bool csr)
{
    int rc;
    if (const uint32_t measure = strat_view(h, strat)) {
        // strategies 3 and 6: the measure is scored here if it is missing, then the round is strategy 2's on that array -- already
        // scored, so the selection is the non-fused one (score_for_selection) -- and round_end runs inside the same view.  (Strategy
        // 6 has scored SDPCUT_EIG with its measure: the rows kernel receives d_eig, the rows are those the score was computed from.)
        if (!h->have_point || !h->d_eig.get()) return sdpcut_fail(h, SDPCUT_ESTATE, "set_candidates and set_point first");
        SDPCUT_NO_PENDING(h);
        if (!(h->scored & measure) && (rc = sdpcut_score(h, measure))) return rc;
        MeasureAsObj view(h, measure);
        rc = round_begin(h, SDPCUT_STRAT_OPT, sel_size, coef_ld, csr);
        if (!rc) h->pend.view = measure;
        return rc;
    }
    rc = check_round_strategy(h, strat);
    if (rc) return rc;
    if (sel_size < 0) return sdpcut_fail(h, SDPCUT_EINVAL, "bad select_round arguments");
    if (!h->have_point || !h->d_eig.get()) return sdpcut_fail(h, SDPCUT_ESTATE, "set_candidates and set_point first");
    if (coef_ld < h->row_len_max || coef_ld > SDPCUT_ROW_LD)
        return sdpcut_fail(h, SDPCUT_EINVAL, "coef_ld must hold the longest row (k + k(k+1)/2) and be <= SDPCUT_ROW_LD");
    SDPCUT_NO_PENDING(h);        // a fused round begun, or a sharded round enqueued and not waited for
    HIP_TRY(h, hipSetDevice(h->device));
    int64_t cap = sel_size < h->N ? sel_size : h->N;
    int stage = 0;               // how far the selection's first pass has got (topk_select_enqueue)
    bool auto_regime = false;
    // SDPCUT_OPT_EXACT_HEAD: the fast scores only filter (exact_head.hip); plain scoring, the selection counts for itself
    const bool exact = cap > 0 && exact_head_applies(h, strat);
    if (!h->exact_suspended) h->stat_exact_last = 0;
    if (exact && exact_first_band(h, cap) > TK_LDSK)
        return sdpcut_fail(h, SDPCUT_EINVAL, "SDPCUT_OPT_EXACT_HEAD: the head plus its band (min(N, sel_size + max(256, sel_size / 8))) must not exceed 8192 entries");
    if (exact) {
        const uint32_t need = strat_need(strat);
        if ((h->scored & need) != need) rc = sdpcut_score(h, need & ~h->scored);
    } else {
        rc = score_for_selection(h, strat, sel_size, cap, strat_need(strat), h->auto_regime, &stage, &auto_regime);
    }
    if (rc) return rc;
    // a launch that skipped the non-violated candidates: d_obj serves the selection enqueued below and nobody else
    const ObjDemoteGuard partial = {h, !exact && h->skip_launched};
    PendingRound &P = h->pend;
    P = PendingRound();
    P.strat = strat; P.sel_size = sel_size; P.cap = cap; P.ld = coef_ld; P.csr = csr;
    P.skipped = partial.on;
    P.exact_band = exact ? exact_first_band(h, cap) : 0;
    if (cap == 0) {   // nothing to generate; round_end still reports the ranking's length / strategy switch
        P.active = true;
        return SDPCUT_OK;
    }
    // one block for everything a round returns: counters | idx | score | lam | rhs | coef | ks
    const RowsLayout y = rows_layout(64, cap, coef_ld);
    rc = ensure_stage(h, y.bytes + 64);
    if (rc) return rc;
    rc = ensure_pinned(h, csr ? csr_layout(cap, coef_ld).bytes : y.bytes);
    if (rc) return rc;
    int64_t *d_idx = (int64_t *)((char *)h->d_stage.get() + y.idx);
    double *d_sc = (double *)((char *)h->d_stage.get() + y.score);
    if (h->timing > 1) HIP_TRY(h, hipEventRecord(h->ev[2], h->stream));
    int64_t *hdr = (int64_t *)h->pinned.get();
    if (csr) hdr[8] = hdr[9] = hdr[10] = 0;
    // fast path: selection and rows are enqueued back to back; the epilogue kernel stores the
    // results directly into the pinned host block (no copy engine); one synchronisation
    const int64_t *d_cnt = nullptr;
    if (exact) {
        rc = exact_head_enqueue(h, strat, sel_size, cap, P.exact_band, d_idx, d_sc, &d_cnt);
        if (rc) return rc;
        rc = 1;
    } else {
        rc = rank_fast_enqueue(h, strat, sel_size, cap, d_idx, d_sc, &d_cnt, stage, auto_regime);
    }
    if (rc < 0) return rc;
    P.fast_tried = rc == 1;
    if (P.fast_tried) {
        if (h->timing > 1) HIP_TRY(h, hipEventRecord(h->ev[3], h->stream));
        // the epilogue's last workgroup publishes this round's serial number in the block's header: the
        // host polls that word instead of waiting for the runtime's completion signal (~5 us earlier)
        P.serial = ++h->round_serial;
        rc = csr ? launch_round_csr(h, cap, d_cnt, cap, d_idx, d_sc, coef_ld, h->pinned.dev(), P.serial)
                 : launch_round_rows(h, cap, d_cnt, d_idx, d_sc, coef_ld, h->pinned.dev(), 64, P.serial);
        if (rc) return rc;
    }
    P.active = true;
    return SDPCUT_OK;
}

// SDPCUT_OPT_EXACT_HEAD: the first band of the pending round P did not prove that it holds the exact head; the same round through
// the widest band (scores, staging and pinned block are in place), under a fresh serial number.
static int round_begin_exact_again(sdpcut_ctx *h, PendingRound &P)
{
    const RowsLayout y = rows_layout(64, P.cap, P.ld);
    int64_t *d_idx = (int64_t *)((char *)h->d_stage.get() + y.idx);
    double *d_sc = (double *)((char *)h->d_stage.get() + y.score);
    int64_t *hdr = (int64_t *)h->pinned.get();
    if (P.csr) hdr[8] = hdr[9] = hdr[10] = 0;
    P.exact_band = exact_widest_band(h);
    const int64_t *d_cnt = nullptr;
    int rc = exact_head_enqueue(h, P.strat, P.sel_size, P.cap, P.exact_band, d_idx, d_sc, &d_cnt);
    if (rc) return rc;
    P.serial = ++h->round_serial;
    return P.csr ? launch_round_csr(h, P.cap, d_cnt, P.cap, d_idx, d_sc, P.ld, h->pinned.dev(), P.serial)
                 : launch_round_rows(h, P.cap, d_cnt, d_idx, d_sc, P.ld, h->pinned.dev(), 64, P.serial);
}

// A CSR assembly into the handle's pinned block, launched here and waited for: header words 8 .. last_word zeroed (10 for the
// plain assembly, 11 for the multi-cut one), a fresh serial number, launch(serial), wait_round_done.
// The look-back of the assembly kernels over lower-indexed workgroups is bounded (rows_dev.h: CSR_SPIN_LIMIT): on a device shared
// with a kernel that blocks it for long it gives up and sets header word 10.  That is a transient condition, not an error of the
// round: by the time the host sees the mark every workgroup of that launch has retired, so ONE more launch over the same head
// (ids and scores still on the device) finds its predecessors' aggregates as soon as they are dispatched.  A give-up that is
// followed by another launch is counted like the selection's fallbacks; after `launches` of them (2; 1 where the caller's own
// launch was the first and has given up) the call fails in the name of `what`, and count_failure says whether that last give-up
// is counted too (the diverse and the multi-cut round always did, the plain round never).
int csr_assemble_wait(sdpcut_ctx *h, int last_word, int launches, bool count_failure, const char *what,
                      const std::function<int(int64_t serial)> &launch)
{
    int64_t *hdr = (int64_t *)h->pinned.get();
    for (;;) {
        for (int w = 8; w <= last_word; ++w) hdr[w] = 0;
        const int64_t serial = ++h->round_serial;
        int rc = launch(serial);
        if (rc) return rc;
        rc = wait_round_done(h, hdr + 7, serial);
        if (rc) return rc;
        if (!hdr[10]) return SDPCUT_OK;
        --launches;
        if (launches > 0 || count_failure) ++h->stat_fallbacks;
        if (launches <= 0) return sdpcut_fail(h, SDPCUT_EHIP, std::string(what) + ": look-back of the row assembly timed out twice");
    }
}

// The plain assembly of the first w entries of a head the host produced (ids and scores in the staging area).
static int csr_head_again(sdpcut_ctx *h, const PendingRound &P, int64_t w, int launches)
{
    const RowsLayout y = rows_layout(64, P.cap, P.ld);
    const int64_t *d_idx = (const int64_t *)((char *)h->d_stage.get() + y.idx);
    const double *d_sc = (const double *)((char *)h->d_stage.get() + y.score);
    return csr_assemble_wait(h, 10, launches, false, "round_csr", [&](int64_t serial) {
        return launch_round_csr(h, P.cap, nullptr, w, d_idx, d_sc, P.ld, h->pinned.dev(), serial);
    });
}

// Rows of the first w entries of a head the host just produced (after the enqueued epilogue ran), into the pinned block.
// CSR: the assembly kernel once more (csr_assemble_wait); padded: cut rows into the staging area, which
// mirrors the pinned block, and one copy.  csr_if_empty: whether a head of no entries still runs the CSR assembly.
static int emit_head(sdpcut_ctx *h, const PendingRound &P, int64_t w, bool csr_if_empty)
{
    if (P.csr) return (w <= 0 && !csr_if_empty) ? 0 : csr_head_again(h, P, w, 2);
    if (w <= 0) return 0;
    const RowsLayout y = rows_layout(64, P.cap, P.ld);
    char *st = (char *)h->d_stage.get();
    const int64_t *d_idx = (const int64_t *)(st + y.idx);
    int rc = launch_cut_rows(h, w, nullptr, d_idx, h->base, (double *)(st + y.lam), (double *)(st + y.coef), P.ld, (double *)(st + y.rhs),
                         nullptr, (int32_t *)(st + y.ks));
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->pinned.get(), h->d_stage.get(), y.bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return 0;
}

static int round_end(sdpcut_ctx *h, const void **block, int64_t *cap_out, int64_t *n_out, int64_t *n_total, int32_t *new_strat,
                     int64_t *counters)
{
    if (!block || !cap_out || !n_out) return sdpcut_fail(h, SDPCUT_EINVAL, "bad select_round arguments");
    if (!h->pend.active) return sdpcut_fail(h, SDPCUT_ESTATE, "no round pending on this handle");
    if (const uint32_t measure = h->pend.view) {
        h->pend.view = 0;
        MeasureAsObj view(h, measure);
        const int rc3 = round_end(h, block, cap_out, n_out, n_total, new_strat, counters);
        if (!rc3 && new_strat) *new_strat = view_strat(measure);
        return rc3;
    }
    PendingRound P = h->pend;
    h->pend.active = false;
    HIP_TRY(h, hipSetDevice(h->device));
    if (P.exact_band > 0 && P.cap > 0) {
        // the verdict of the band rule arrives with the block (hdr[4]): exact -- the ordinary code below finds its round complete;
        // a band that did not prove itself -- once more with the widest one (a second wait); else the ordinary round, whole
        int rc = wait_round_done(h, (const int64_t *)h->pinned.get() + 7, P.serial);
        if (rc) return rc;
        int v = exact_head_verdict(h, (const int64_t *)h->pinned.get(), P.exact_band);
        if (v == 1) {
            ++h->stat_exact_retries;
            rc = round_begin_exact_again(h, P);
            if (rc) return rc;
            rc = wait_round_done(h, (const int64_t *)h->pinned.get() + 7, P.serial);
            if (rc) return rc;
            v = exact_head_verdict(h, (const int64_t *)h->pinned.get(), P.exact_band);
        }
        if (v != 0) {
            ++h->stat_exact_gave_up;
            h->exact_suspended = true;
            rc = round_begin(h, P.strat, P.sel_size, P.ld, P.csr);
            h->exact_suspended = false;
            if (rc) return rc;
            P = h->pend;
            h->pend.active = false;
        } else {
            h->stat_exact_last = 1;
        }
    }
    if (P.skipped) {
        // SDPCUT_OPT_SKIP_NONVIOLATED: the enqueued selection is the answer only if it ran in the strong regime and was not void --
        // nothing else of the round reads the measure of a candidate that is not violated.  Every entry visited (resolved on the
        // device, or by the host below), or a selection that gave up: complete d_obj and begin the round again -- scored now, it
        // takes the ordinary road under a fresh serial number.
        // (fast_tried and cap > 0 hold for every skipped round -- score_for_selection lets the launch count, and so skip, only for a
        // head rank_fast_mode serves, which rank_fast_enqueue then enqueues; were they not to, the round is simply begun again)
        bool keep = false;
        if (P.fast_tried && P.cap > 0) {
            int rc = wait_round_done(h, (const int64_t *)h->pinned.get() + 7, P.serial);
            if (rc) return rc;
            const int64_t *c = (const int64_t *)h->pinned.get();
            keep = !c[4] && c[6] == TK_MODE_STRONG && c[0] >= (P.sel_size < h->N ? P.sel_size : h->N);
            h->stat_nn_skipped = h->N - c[1];
            // a selection that gave up is a fallback whichever road answers it (until the give-up tests this one went uncounted:
            // the round begun again below finds a clean header)
            if (c[4] == 1) ++h->stat_fallbacks;      // (2, the tie group, is no fallback: the round begun again splits it)
        }
        if (!keep) {
            int rc = obj_complete(h);
            if (rc) return rc;
            rc = round_begin(h, P.strat, P.sel_size, P.ld, P.csr);
            if (rc) return rc;
            P = h->pend;
            h->pend.active = false;
        }
    }
    const int strat = P.strat;
    const int64_t sel_size = P.sel_size, cap = P.cap;
    *n_out = 0;
    *cap_out = cap;
    *block = nullptr;
    if (cap == 0) return sdpcut_rank(h, strat, sel_size, 0, nullptr, nullptr, n_total, new_strat, counters);
    const RowsLayout y = rows_layout(64, cap, P.ld);
    int64_t *d_idx = (int64_t *)((char *)h->d_stage.get() + y.idx);
    double *d_sc = (double *)((char *)h->d_stage.get() + y.score);
    int64_t *hdr = (int64_t *)h->pinned.get();
    int rc;
    int64_t w = 0;
    bool have = false;
    if (P.fast_tried) {
        rc = wait_round_done(h, hdr + 7, P.serial);
        if (rc) return rc;
        have = rank_fast_finish(h, strat, sel_size, cap, (const int64_t *)h->pinned.get(), &w, n_total, new_strat, counters) != 0;
        if (have && P.csr && hdr[10] && w > 0) {      // the enqueued assembly gave up its look-back: once more, see csr_assemble_wait
            ++h->stat_fallbacks;
            rc = csr_head_again(h, P, w, 1);
            if (rc) return rc;
        }
    }
    ++h->stat_rounds;
    bool resorted = false;      // the head in d_idx / d_sc was produced after the enqueued epilogue ran: launch it again
    if (P.fast_tried && !have && strat == SDPCUT_STRAT_COMB && hdr[4] == 2 && hdr[6] == TK_MODE_COMBALL) {
        // the threshold tie group of the every-entry-visited ranking does not fit the sort buffers (a structured LP vertex):
        // cut it by its secondary key with two more selections (topk.hip: topk_tie_split) instead of sorting the full list
        int64_t c7[7];
        for (int i = 0; i < 7; ++i) c7[i] = hdr[i];
        rc = topk_tie_split(h, cap, d_idx, d_sc, nullptr);
        if (rc < 0) return rc;
        if (rc == 0) {
            c7[4] = 0;
            have = rank_fast_finish(h, strat, sel_size, cap, c7, &w, n_total, new_strat, counters) != 0;
            resorted = have;
        }
    }
    if (P.fast_tried && !have && hdr[4]) ++h->stat_fallbacks;
    if (resorted) {
        if (h->timing > 1) HIP_TRY(h, hipEventRecord(h->ev[3], h->stream));
        rc = emit_head(h, P, w, true);       // (the CSR assembly runs here whatever w is)
        if (rc) return rc;
    }
    if (!have) {
        // general path (full sorts; the combined scan visiting every entry, or heads > 8192)
        // (the fast attempt above already counted the strong candidates: with its count as hint there is no second attempt; a VOID
        // attempt has no count to hand on -- hint -1 -- and rank_on_device makes its own, which answers unless it is void as well)
        if (P.exact_band > 0 && h->stat_exact_last) {      // (never seen: an exact head's counters always answer) nothing half-exact
            h->stat_exact_last = 0;
            ++h->stat_exact_gave_up;
        }
        const int64_t *c5 = (const int64_t *)h->pinned.get();
        const int64_t hint = (P.fast_tried && strat == SDPCUT_STRAT_COMB && !c5[4]) ? c5[0] : -1;
        rc = rank_on_device(h, strat, sel_size, cap, d_idx, d_sc, &w, n_total, new_strat, counters, hint);
        if (rc) return rc;
        if (h->timing > 1) HIP_TRY(h, hipEventRecord(h->ev[3], h->stream));
        rc = emit_head(h, P, w, false);
        if (rc) return rc;
    }
    *n_out = w;
    *block = h->pinned.get();
    return SDPCUT_OK;
}

static int round_impl(sdpcut_ctx *h, int strat, int64_t sel_size, int32_t coef_ld, bool csr, const void **block,
                      int64_t *cap_out, int64_t *n_out, int64_t *n_total, int32_t *new_strat, int64_t *counters)
{
    if (!block || !cap_out || !n_out) return sdpcut_fail(h, SDPCUT_EINVAL, "bad select_round arguments");
    int rc = round_begin(h, strat, sel_size, coef_ld, csr);
    if (rc) return rc;
    return round_end(h, block, cap_out, n_out, n_total, new_strat, counters);
}

extern "C" {

int sdpcut_select_round_view(sdpcut_handle h, int strat, int64_t sel_size, int32_t coef_ld, const void **block,
                             int64_t *cap_out, int64_t *n_out, int64_t *n_total, int32_t *new_strat, int64_t *counters)
{
    if (!h) return SDPCUT_EINVAL;
    return round_impl(h, strat, sel_size, coef_ld, false, block, cap_out, n_out, n_total, new_strat, counters);
}

int sdpcut_round_csr_begin(sdpcut_handle h, const double *vars_values, int strat, int64_t sel_size)
{
    if (!h) return SDPCUT_EINVAL;
    int rc;
    if (vars_values && (rc = sdpcut_set_point(h, vars_values))) return rc;
    return round_begin(h, strat, sel_size, h->row_len_max, true);
}

int sdpcut_round_csr_end(sdpcut_handle h, sdpcut_round_csr_t *out)
{
    if (!h) return SDPCUT_EINVAL;
    if (!out) return sdpcut_fail(h, SDPCUT_EINVAL, "out is NULL");
    std::memset(out, 0, sizeof(*out));
    if (!h->pend.active || !h->pend.csr) return sdpcut_fail(h, SDPCUT_ESTATE, "no sdpcut_round_csr_begin pending on this handle");
    const void *block = nullptr;
    out->row_ld = h->pend.ld;
    int rc = round_end(h, &block, &out->cap, &out->n_out, &out->n_total, &out->new_strat, out->counters);
    if (rc) return rc;
    if (block && out->cap != 0) csr_out_from_block(block, out);
    return SDPCUT_OK;
}

int sdpcut_round_csr(sdpcut_handle h, const double *vars_values, int strat, int64_t sel_size, sdpcut_round_csr_t *out)
{
    if (!h) return SDPCUT_EINVAL;
    if (!out) return sdpcut_fail(h, SDPCUT_EINVAL, "out is NULL");
    int rc = sdpcut_round_csr_begin(h, vars_values, strat, sel_size);
    if (rc) { std::memset(out, 0, sizeof(*out)); return rc; }
    return sdpcut_round_csr_end(h, out);
}

int sdpcut_round_view(sdpcut_handle h, const double *vars_values, int strat, int64_t sel_size, int32_t coef_ld,
                      const void **block, int64_t *cap_out, int64_t *n_out, int64_t *n_total, int32_t *new_strat,
                      int64_t *counters)
{
    int rc = sdpcut_set_point(h, vars_values);
    if (rc) return rc;
    return sdpcut_select_round_view(h, strat, sel_size, coef_ld, block, cap_out, n_out, n_total, new_strat, counters);
}

int sdpcut_select_round(sdpcut_handle h, int strat, int64_t sel_size, int32_t coef_ld, int64_t *idx_out,
                        double *score_out, double *lam_min, double *coef, double *rhs, int32_t *ks, int64_t *n_out,
                        int64_t *n_total, int32_t *new_strat, int64_t *counters)
{
    if (!h) return SDPCUT_EINVAL;
    if (sel_size < 0 || (sel_size > 0 && (!idx_out || !score_out || !lam_min || !coef || !rhs || !ks)) || !n_out)
        return sdpcut_fail(h, SDPCUT_EINVAL, "bad select_round arguments");
    const void *block = nullptr;
    int64_t cap = 0;
    int rc = sdpcut_select_round_view(h, strat, sel_size, coef_ld, &block, &cap, n_out, n_total, new_strat, counters);
    if (rc) return rc;
    if (*n_out > 0) {
        const size_t ww = (size_t)*n_out;
        const RowsLayout y = rows_layout(64, cap, coef_ld);
        const char *q = (const char *)block;
        std::memcpy(idx_out, q + y.idx, ww * 8);
        std::memcpy(score_out, q + y.score, ww * 8);
        std::memcpy(lam_min, q + y.lam, ww * 8);
        std::memcpy(rhs, q + y.rhs, ww * 8);
        std::memcpy(coef, q + y.coef, ww * 8 * (size_t)coef_ld);
        std::memcpy(ks, q + y.ks, ww * 4);
    }
    return SDPCUT_OK;
}

} // extern "C"
