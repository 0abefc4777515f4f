// Which route a top-k selection takes: the modes, the limits the host needs and ONE pure function from plain values to a plan.
// Plain C++, no HIP: the selection's host code (topk.hip), the question the scoring asks before it runs (topk_fuse_ok) and
// tests/test_topk_route.py (which compiles this header alone) all read the policy here and nowhere else.
#pragma once
#include <stdint.h>

#include "../../include/sdpcut.h"

#define TK_THREADS 256
#define TK_MAXBLK 1024   // most workgroups a selection pass is launched with (blk_eq / blk_gt slots)
#define TK_LDSK 8192     // heads whose compacted superset (keys AND indices) fits the merge kernel's LDS
#define TK_MAXK 16384    // largest head: the merge keeps the keys in LDS and reads indices only on ties
#define TK_TILE 512      // entries of a sort tile (tk_tilesort_kernel)
// tk_countrank_kernel: every group of 64 compacted entries is ranked by TK_CR_SLICES waves, one per slice of the scanned keys
// (a multiple of the four waves of a workgroup)
#ifndef TK_CR_SLICES
#define TK_CR_SLICES 32
#endif
#define TK_CACHE 4096    // keys of a workgroup's chunk kept in LDS between the passes (32 KB)
// lists of at most TK_SMALLSEL_N candidates with a head of at most TK_LDSK: selection by ONE workgroup, keys in LDS (tk_smallsel_kernel)
#ifndef TK_SMALLSEL
#define TK_SMALLSEL 1
#endif
#ifndef TK_SMALLSORT
#define TK_SMALLSORT 1     // ... and, for heads of one tile at most, sorted and emitted by it too (ONE launch for the round's selection)
#endif
#define TK_SMALLSEL_N 12288
// Which lists the one-workgroup selection takes (measured, profiles/r04_short_list_selection.txt: fused rounds on lists of 64 ..
// 65 536 candidates, both paths alternating on one box).  Below ~3000 candidates sorting every class member costs less than
// selecting first (two tiles at most); above 8192 the multi-workgroup passes win again -- except in the combined strategy, whose
// tie-aware sort of a whole class is dearer: there 2048 .. 12 288.
#define TK_SMALLSEL_LO 3072
#define TK_SMALLSEL_HI 8192
#define TK_SMALLSEL_COMB_LO 2048
#define TK_SMALLSEL_COMB_HI 12288
// ... and with the sort inside (heads of one tile at most, no shard record to write behind the head): lists of at most 4096
// candidates -- ONE launch instead of three, 55 -> 47 us per combined round on 64 candidates, 68 -> 59 on 2048, 70 -> 66 on 4096;
// beyond that the four waves that sort lose to the tile-sort launch what the saved hand-offs gain (same evidence file)
#define TK_SMALLSORT_N 4096

// lists shorter than this do not count the fine histogram of their selection (topk_dev.h): their heads come from the one-workgroup
// selections or from passes over a few thousand keys, and their epilogues are too small to zero 34 KB more
#define SDPCUT_PF_MIN_N 32768

// 4: combined strategy when the scan visits every entry -- the key is the new score of
// cut_select_qp.py:606-623, ties between equal new scores go by obj_improve, then index
// 5: combined strategy, regime resolved ON THE DEVICE by the first pass: STRONG if the score kernels
// counted at least `sel` strong candidates (counters[5]), else COMBALL -- one selection, no host
// round trip in either regime
enum { TK_MODE_FEAS = 1, TK_MODE_OPT = 2, TK_MODE_STRONG = 3, TK_MODE_COMBALL = 4, TK_MODE_COMBAUTO = 5 };

// One value per row of the table in DESIGN.md section 5; the first row that matches wins.
enum TkRoute {
    TK_ROUTE_SMALLSORT = 1,   // tk_smallsel_kernel<true> alone: selection, sort and emission in one launch       (topk_small.hip)
    TK_ROUTE_SMALLSEL = 2,    // tk_smallsel_kernel<false>, sort tail                                              (topk_small.hip)
    TK_ROUTE_SMALL = 3,       // tk_small_kernel (the whole class goes to the sort), sort tail                     (topk_small.hip)
    TK_ROUTE_ONFLY = 4,       // tk_refine_kernel<true>: digit 0 counted by the score kernels, no key array         (topk_passes.hip)
    TK_ROUTE_COOP = 5,        // key pass, tk_refine_kernel<false> launched cooperatively, sort tail               (topk_passes.hip)
    TK_ROUTE_FUSED = 6,       // key pass, tk_refine_kernel<false>, sort tail                                      (topk_passes.hip)
    TK_ROUTE_DIGITS = 7,      // key pass, tk_hist_kernel x 7, tk_count_kernel, tk_write_kernel, sort tail (topk_passes.hip, topk_compact.hip)
    // tk_refine_kernel<true, true>: TK_ROUTE_ONFLY whose launch first looks at what the device alone knows -- the regime and the
    // overflow flag of the emitted list -- and, in the strong regime without an overflow, compacts the head's superset from the
    // (key, index) pairs the skipping score launch appended instead of rebuilding 10^6 keys from the scores; otherwise it is
    // TK_ROUTE_ONFLY's code from there on, same result                                                              (topk_passes.hip)
    TK_ROUTE_EMITTED = 8
};

struct TkRouteIn {
    int64_t n = 0, k = 0;            // candidates of the list, entries of the head
    int mode = TK_MODE_FEAS;
    // 0: fresh selection; 1: the workspace has been handed out by topk_begin already (the score kernels left their strong count
    // in it); 3: the score kernels also counted the leading digit of the keys and the violated / positive candidates
    int stage = 0;
    bool fused_tail = true, coop_launch = false;      // SDPCUT_OPT_FUSED_TAIL, SDPCUT_OPT_COOP_LAUNCH
    bool shard_rec = false;                           // a shard record is written behind the head
    bool prefilter = true, pf_counted = false;        // SDPCUT_OPT_PREFILTER; this round's score launches counted the fine histogram
    int64_t tk_coresident = 256;                      // workgroups of tk_refine_kernel the device holds at once
    bool prekeys = false;                             // the keys exist already (tk_prekeys_kernel is the key pass): rows 5-7 only
    bool raw = false;                                 // the head's scores are emitted as raw key images (big-head merge only)
    bool smallsel = TK_SMALLSEL != 0, smallsort = TK_SMALLSORT != 0;
    bool count_rank = true;                           // SDPCUT_OPT_COUNT_RANK
    bool emitted = false;                             // this round's (skipping) score launch appended its strong members to the emitted list
};

struct TkPlan {
    int err = 0;                  // 0, or the SDPCUT_E* the selection is refused with (msg says why)
    const char *msg = nullptr;
    int route = 0;                // TkRoute
    int64_t maxk = 0;             // what the sort buffers of this head hold: an early stop compacts up to maxk entries
    // sort tail (none behind TK_ROUTE_SMALLSORT): tk_countrank_kernel<sort_tie> alone where count_rank says so, else
    // tk_tilesort_kernel<sort_tie>, then tk_mergerank_kernel<sort_tie> or, for big heads, tk_mergerank_big_kernel<sort_tie != 0>
    int sort_tie = 0;             // 0 ties by index, 1 COMBALL (by obj_improve, then index), 2 COMBAUTO (decided on the device)
    bool big_merge = false;       // heads of 8193 .. 16384: keys-only merge
    // ranks by counting in ONE launch (topk_sort.hip): heads that fit TK_LDSK, scores emitted as scores, no shard record behind
    // the head (its header and padding are written by tk_mergerank_kernel)
    bool count_rank = false;
    int ntiles = 0;               // grid of the tile sort; the merge runs ntiles * TK_TILE / TK_THREADS workgroups
    int grid_keys = 0;            // grid of the key pass (tk_keys_kernel / tk_prekeys_kernel)
    int grid_pass = 0;            // grid of the digit passes, the count and the compaction
    int64_t chunk = 0;            // keys per workgroup of the passes, a multiple of TK_THREADS
    int64_t pf_k = 0;             // TK_ROUTE_ONFLY: head size for the direct selection from the fine histogram, 0 = digit passes
};

static inline TkPlan tk_refuse(TkPlan p, int err, const char *msg)
{
    p.err = err;
    p.msg = msg;
    return p;
}

static inline TkPlan tk_route(const TkRouteIn &in)
{
    TkPlan p;
    const int64_t n = in.n, k = in.k;
    if (k < 1 || k > TK_MAXK || n < 1) return tk_refuse(p, SDPCUT_EINVAL, "top-k select: k out of range");
    if (in.mode == TK_MODE_COMBAUTO && in.stage != 1 && in.stage != 3) return tk_refuse(p, SDPCUT_ESTATE, "top-k select: no strong count");
    const bool digit_done = in.stage == 3;      // the score kernels counted digit 0; no key array (tk_refine_kernel<true>)
    const bool comb = in.mode == TK_MODE_COMBAUTO || in.mode == TK_MODE_COMBALL;
    const bool fresh = !digit_done && !in.prekeys;      // the one-workgroup routes build their own keys
    p.maxk = k <= TK_LDSK ? TK_LDSK : TK_MAXK;
    p.big_merge = p.maxk > TK_LDSK;
    p.sort_tie = in.mode == TK_MODE_COMBAUTO ? 2 : (in.mode == TK_MODE_COMBALL ? 1 : 0);
    p.ntiles = (int)(p.maxk / TK_TILE);
    const int64_t nb = (n + TK_THREADS - 1) / TK_THREADS;
    p.grid_keys = (int)(nb < TK_MAXBLK ? nb : TK_MAXBLK);
    // Workgroups of the passes: one LDS-cached chunk of TK_CACHE keys each, as many as can be RESIDENT together -- the
    // fused kernel's grid barriers (masses of equal keys only) need that, and its waits are bounded anyway.  A fixed
    // grid of 256 read the 200 MB of a 1.25e7-candidate shard at 18 % of the HBM rate: the loads in
    // flight, not the bandwidth, were the limit.
    const int64_t want = (n + TK_CACHE - 1) / TK_CACHE;
    const int64_t cap = in.fused_tail ? (in.tk_coresident < TK_MAXBLK ? in.tk_coresident : TK_MAXBLK) : TK_MAXBLK;
    p.grid_pass = (int)(want < 1 ? 1 : (want < cap ? want : cap));
    // (tk_coresident < 1 switches fused_tail off when the workspace is made, ensure_topk_ws: an empty grid is never launched)
    p.chunk = p.grid_pass < 1 ? 0 : ((n + p.grid_pass - 1) / p.grid_pass + TK_THREADS - 1) / TK_THREADS * TK_THREADS;

    if (fresh && in.smallsel && in.smallsort && k <= TK_TILE && n <= TK_SMALLSORT_N && !in.shard_rec) {
        p.route = TK_ROUTE_SMALLSORT;
        return p;
    }
    // (a head of more than a quarter of the list -- the 5000 of a 7899-candidate QCQP cover -- is not worth selecting: the
    // threshold lies deep in the list, five or six passes and the cut by index, 32 us where sorting the whole class takes 39 - 14)
    if (fresh && in.smallsel && k <= TK_LDSK && n <= TK_SMALLSEL_N && 4 * k <= n &&
        (comb ? (n > TK_SMALLSEL_COMB_LO && n <= TK_SMALLSEL_COMB_HI) : (n > TK_SMALLSEL_LO && n <= TK_SMALLSEL_HI)))
        p.route = TK_ROUTE_SMALLSEL;
    // Lists that fit the sort buffers whole (most of the reference's BoxQP / QCQP instances) need no radix passes
    else if (fresh && n <= p.maxk)
        p.route = TK_ROUTE_SMALL;
    else if (digit_done) {
        if (!in.fused_tail) return tk_refuse(p, SDPCUT_ESTATE, "top-k select: no key pass to continue from");
        p.route = TK_ROUTE_ONFLY;
        p.pf_k = (in.prefilter && in.pf_counted && n >= SDPCUT_PF_MIN_N) ? k : 0;
        // the list holds the strong class and nothing else: only a selection that may resolve to it reads it, and the sort behind
        // must be the one that takes any superset in any order (heads that fit TK_LDSK, no shard record)
        if (in.emitted && in.mode == TK_MODE_COMBAUTO && !in.shard_rec && k <= TK_LDSK) p.route = TK_ROUTE_EMITTED;
    } else if (in.fused_tail)
        p.route = in.coop_launch ? TK_ROUTE_COOP : TK_ROUTE_FUSED;      // cooperative: the runtime guarantees the co-residency (+20 us per launch)
    else      // one launch per digit, no wait anywhere inside a kernel: the path that always answers
        p.route = TK_ROUTE_DIGITS;
    p.count_rank = in.count_rank && !p.big_merge && !in.raw && !in.shard_rec;
    // big heads (8193 .. 16384): keys-only merge; the device-resolved regime never asks for them
    if (p.big_merge && in.mode == TK_MODE_COMBAUTO) return tk_refuse(p, SDPCUT_EINVAL, "top-k select: head too long for this mode");
    if (!p.big_merge && in.raw) return tk_refuse(p, SDPCUT_EINVAL, "top-k select: raw output needs the big-head merge");
    return p;
}

// May the score kernels count the leading digit for a head of k entries (ScoreFuse, stage 3)?  Exactly when a fresh selection
// of this list would run the key pass and ONE plain launch of the fused kernel: stage 3 replaces that key pass.  The one-workgroup
// routes build their own keys (nothing to count), and the cooperative and launch-per-digit routes have no on-the-fly variant.
// comb: the selection will run in a tie-aware combined mode (regime resolved on the device).
static inline bool tk_fuse_ok(TkRouteIn in, bool comb)
{
    in.mode = comb ? TK_MODE_COMBALL : TK_MODE_FEAS;
    in.stage = 0;
    in.prekeys = in.raw = false;
    const TkPlan p = tk_route(in);
    return p.err == 0 && p.route == TK_ROUTE_FUSED;
}
