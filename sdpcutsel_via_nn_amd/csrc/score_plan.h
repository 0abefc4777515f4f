// The rules of a scoring launch as pure functions from plain values: the shapes of the shipped networks (NetShape), how the
// MFMA kernel's work is split over a class (score_plan), how far down its table a workgroup reports (pf_mloc_rule) and which
// form a call of launch_score takes or why it is refused (score_form).
// Plain C++, no HIP: the launchers (score.hip, score_mfma.hip, score_alt.hip, eig.hip) and tests/test_score_plan.py (which
// compiles this header alone) read the rules here and nowhere else.
#pragma once
#include <stdint.h>

#include "../../include/sdpcut.h"
#include "topk_route.h"      // TK_MODE_*

// ---- the networks the MFMA / VALU kernels are instantiated for -----------------------------------------------------------------
// H hidden width, NH hidden (tansig) layers of the network of K-variable candidates
template <int K> struct NetShape;
template <> struct NetShape<2> { static constexpr int H = 64, NH = 3; };
template <> struct NetShape<3> { static constexpr int H = 50, NH = 3; };
template <> struct NetShape<4> { static constexpr int H = 50, NH = 3; };
template <> struct NetShape<5> { static constexpr int H = 64, NH = 4; };

// is a network of this width and depth the one size class K's kernels are compiled for?
static inline bool net_shape_is(int K, int width, int n_hidden)
{
    switch (K) {
    case 2: return width == NetShape<2>::H && n_hidden == NetShape<2>::NH;
    case 3: return width == NetShape<3>::H && n_hidden == NetShape<3>::NH;
    case 4: return width == NetShape<4>::H && n_hidden == NetShape<4>::NH;
    case 5: return width == NetShape<5>::H && n_hidden == NetShape<5>::NH;
    default: return false;
    }
}

// J = 16-candidate column tiles per pass of the MFMA kernel (score_mfma.hip).  2 (default): every weight fragment feeds two MFMAs,
// ~230 registers, two waves per SIMD.  1: half the accumulator state (<= 168 registers: three waves per SIMD), twice the fragment
// loads and tail evaluations per candidate -- the experiment of VERDICT r2 item 4, measured in DESIGN.md section 5.
#ifndef SDPCUT_MFMA_J
#define SDPCUT_MFMA_J 2
#endif
#ifndef SDPCUT_MFMA_J_K2
#define SDPCUT_MFMA_J_K2 SDPCUT_MFMA_J
#endif
#ifndef SDPCUT_MFMA_J_K3
#define SDPCUT_MFMA_J_K3 SDPCUT_MFMA_J
#endif
#ifndef SDPCUT_MFMA_J_K4
#define SDPCUT_MFMA_J_K4 SDPCUT_MFMA_J
#endif
#ifndef SDPCUT_MFMA_J_K5
#define SDPCUT_MFMA_J_K5 SDPCUT_MFMA_J
#endif
#ifndef SDPCUT_MFMA_J1_WAVES
#define SDPCUT_MFMA_J1_WAVES 3
#endif
constexpr int mfma_cols(int K) { return K == 2 ? SDPCUT_MFMA_J_K2 : K == 3 ? SDPCUT_MFMA_J_K3 : K == 4 ? SDPCUT_MFMA_J_K4 : SDPCUT_MFMA_J_K5; }

// ---- the work split of the MFMA kernel over one size class ---------------------------------------------------------------------
// workgroups per CU launched for the MFMA kernel (2 are resident at a time: 2 waves / SIMD)
#ifndef SDPCUT_MFMA_BLOCKS_PER_CU
#define SDPCUT_MFMA_BLOCKS_PER_CU 8
#endif

static inline int grid_for(int n_cu, int64_t ntiles, int per_cu)
{
    int64_t cap = (int64_t)n_cu * per_cu;
    int64_t g = ntiles < cap ? ntiles : cap;
    return (int)(g < 1 ? 1 : g);
}

#ifndef SDPCUT_PF_SCORE_KMASK
#define SDPCUT_PF_SCORE_KMASK (1 << 3)      // candidate sizes whose score kernel counts the fine histogram (bit k; 0: none; see score_mfma_body)
#endif
constexpr bool pf_score_k(int k) { return ((SDPCUT_PF_SCORE_KMASK >> k) & 1) != 0; }

// How far down its table a workgroup of `per_wg` candidates reports (TopkWs::pf_tab, topk_dev.h): to its m-th largest member,
// m = 24 + eight times its expected share E of a head of head_k out of n_total candidates.  A workgroup with MORE members of the
// head than that makes the selection fall back to its radix passes (the floor check).  For candidates in random order that never
// happens (a Poisson variable of mean 2.6 reaching 45); real covers are enumerated index set by index set, neighbours share
// variables and scores, and the head clusters: spar125-075-1 dim 4 has workgroups with > 18 of the 5000 (8 + 4 E failed there).
// Reporting more costs little: ~45 atomics per workgroup over a few hundred addresses.  0: no fine histogram (no head, or
// a table counter could overflow its 16 bits).
// (8 E is exact -- a scaling by a power of two -- so 24 + (8 head_k) per_wg / n_total, as the eigenvalue launch used to write it,
// is the same double.)
static inline int pf_mloc_rule(int64_t head_k, int64_t per_wg, int64_t n_total)
{
    if (head_k <= 0 || per_wg >= 60000 || n_total < 1) return 0;
    const double share = (double)head_k * (double)per_wg / (double)n_total;
    const double m = 24.0 + 8.0 * share;
    return m > 60000.0 ? 60000 : (int)(m + 0.999);
}

// The balanced tail round (see score_mfma_body): for lists whose last round-robin round would be at least 90 % full
// -- every resident slot then pays a whole strip for it -- the round is split evenly instead, three or four column tiles per wave,
// the four waves of a workgroup alike.  Emptier last rounds are left alone: the two waves of a SIMD share its issue slots, the
// dispatcher fills the gaps with the short workgroups, and a partial strip pays phase A for 64 lanes whatever it holds.  Measured
// (k = 3, this rule against none, profiles/r04_balanced_tail.txt): kernel time over the list length is a plateau up to a fill of
// 0.875 and steps up at 0.9; with the split the step becomes a ramp: 10^6 candidates (0.907) 302 -> 295 us, 0.95: 303 -> 300;
// forced at 0.75-0.875 the split LOSES 2-10 us, hence the threshold; the same at two and three full rounds.
#ifndef SDPCUT_BALANCED_TAIL
#define SDPCUT_BALANCED_TAIL 1
#endif
#ifndef SDPCUT_BALANCED_TAIL_MIN_FILL_PCT
#define SDPCUT_BALANCED_TAIL_MIN_FILL_PCT 90
#endif

// What a launch of the MFMA kernel over a class of n candidates looks like (the fields go into ScoreArgs as they are, the launch
// over all classes sums the grids).
struct ScorePlan {
    int grid = 1;              // workgroups (of four waves)
    int32_t strip = 64;        // candidates per strip of a wave, 64 or 32
    // candidates [0, rr_end) go round-robin in whole strips; the rest -- less than one strip per wave -- is split EVENLY: wave g
    // takes tail_hi (g < tail_nhi) or tail_lo column tiles of 16 candidates from rr_end on.  rr_end = n, tail_hi = tail_lo = 0: no tail
    int64_t rr_end = 0, tail_nhi = 0;
    int32_t tail_hi = 0, tail_lo = 0;
    int32_t pf_mloc = 0;       // pf_mloc_rule of a workgroup's share; 0: the launch does not count the fine histogram
    int32_t spread = 0;        // the four waves of a workgroup take strips from four distant quarters of the list
};

// n >= 1 candidates of size K on a device of n_cu CUs; fused: the launch counts for a selection (ScoreFuse) with a head of fuse_k
// out of n_total candidates.
static inline ScorePlan score_plan(int64_t n, int n_cu, int K, int64_t n_total, int64_t fuse_k, bool fused)
{
    ScorePlan p;
    p.grid = grid_for(n_cu, (n + 255) / 256, SDPCUT_MFMA_BLOCKS_PER_CU);
    if (n <= 32 * (int64_t)n_cu * 4 * 2) {      // part-empty device: one two-tile pass per wave
        p.strip = 32;
        p.grid = (int)(((n + 31) / 32 + 3) / 4);
    }
    p.rr_end = n;
    if (SDPCUT_BALANCED_TAIL && p.strip == 64) {
        const int64_t W = (int64_t)p.grid * 4, round = W * 64;
        const int64_t R = n / round, rem = n - R * round;
        const int64_t tiles = (rem + 15) / 16;
        if (R >= 1 && 100 * rem >= SDPCUT_BALANCED_TAIL_MIN_FILL_PCT * round) {
            const int64_t lo = tiles / W;      // 3 (a remainder of a whole round is R + 1 rounds)
            p.rr_end = R * round;
            p.tail_lo = (int32_t)lo;
            p.tail_hi = (int32_t)lo + 1;
            p.tail_nhi = (tiles - lo * W + 3) / 4 * 4;
        }
    }
    p.pf_mloc = fused && pf_score_k(K) ? pf_mloc_rule(fuse_k, (n + p.grid - 1) / p.grid, n_total) : 0;
    p.spread = p.pf_mloc > 0 && n <= (int64_t)p.grid * 4 * p.strip;
    return p;
}

// ---- the work split of the skipping kernel (score_mfma_skip_kernel) --------------------------------------------------------------
// The fused scoring launch of a combined round (FUSE = TK_MODE_STRONG) runs the MLP only for violated candidates: a wave packs
// them into a private queue that carries over from strip to strip and runs a pass per 32 queued.  Packing pays with the number
// of strips a wave sees, so the launch has fewer, longer-lived waves than score_plan's: SDPCUT_SKIP_BLOCKS_PER_CU workgroups per
// CU (2 = one resident generation).  On the violated pattern of the 10^6-candidate benchmark list the model of passes gives
// 0.908 of today's at 8 workgroups per CU (1.9 strips per wave), 0.878 at 4, 0.862 at 2 (7.6 strips).
#ifndef SDPCUT_SKIP_KMASK
#define SDPCUT_SKIP_KMASK (1 << 3)      // candidate sizes with a skipping instantiation (bit k; 0: none)
#endif
constexpr bool skip_k(int k) { return ((SDPCUT_SKIP_KMASK >> k) & 1) != 0; }
#ifndef SDPCUT_SKIP_BLOCKS_PER_CU
#define SDPCUT_SKIP_BLOCKS_PER_CU 2
#endif
// most strips per wave a forced skip (option value 2) aims at on a list that leaves the device part-empty
#define SDPCUT_SKIP_FORCED_STRIPS 4

// Does the skipping kernel serve a class of n candidates of size K?  opt = SDPCUT_OPT_SKIP_NONVIOLATED: 0 never; 1 where
// score_plan uses strips of 64 (a part-empty device runs one pass per wave and has nothing to pack) and a workgroup's share still
// fits the 16-bit counters of the fine histogram (pf_mloc_rule); 2 whatever the length (tests).
static inline bool score_skip_applies(int64_t n, int n_cu, int K, int opt)
{
    if (!skip_k(K) || opt == 0 || n < 1) return false;
    if (opt == 2) return true;
    return n > 32 * (int64_t)n_cu * 4 * 2 && n < 59000 * (int64_t)n_cu * SDPCUT_SKIP_BLOCKS_PER_CU;
}

// The plan of the skipping launch over n >= 1 candidates; the fields mean what they mean in score_plan.  Strips of 64 round-robin
// over the whole rounds, the last partial round always split evenly in column tiles (there is no later generation of workgroups
// to fill the gaps).  force: at most ceil(strips / SDPCUT_SKIP_FORCED_STRIPS) waves, so that a short list still hands a wave
// several strips.
static inline ScorePlan score_plan_skip(int64_t n, int n_cu, int K, int64_t n_total, int64_t fuse_k, bool force)
{
    ScorePlan p;
    p.strip = 64;
    const int64_t strips = (n + 63) / 64;
    int64_t waves = (int64_t)n_cu * SDPCUT_SKIP_BLOCKS_PER_CU * 4;
    if (force) {
        const int64_t w = (strips + SDPCUT_SKIP_FORCED_STRIPS - 1) / SDPCUT_SKIP_FORCED_STRIPS;
        waves = w < waves ? w : waves;
    }
    waves = strips < waves ? strips : waves;
    p.grid = (int)((waves + 3) / 4 < 1 ? 1 : (waves + 3) / 4);
    p.rr_end = n;
    const int64_t W = (int64_t)p.grid * 4, round = W * 64;
    const int64_t R = n / round, rem = n - R * round;
    if (R >= 1 && rem > 0) {
        const int64_t tiles = (rem + 15) / 16, lo = tiles / W;      // lo <= 4, and 4 only with tail_nhi = 0: rem is less than a round
        p.rr_end = R * round;
        p.tail_lo = (int32_t)lo;
        p.tail_hi = (int32_t)lo + 1;
        p.tail_nhi = (tiles - lo * W + 3) / 4 * 4;
    }
    p.pf_mloc = pf_score_k(K) ? pf_mloc_rule(fuse_k, (n + p.grid - 1) / p.grid, n_total) : 0;
    p.spread = 0;
    return p;
}

// ---- the form of a scoring call ------------------------------------------------------------------------------------------------
enum ScoreFormKind {
    SCORE_FORM_EIG = 1,     // flags == SDPCUT_EIG: the eigenvalue-only kernel, one launch over all classes (eig.hip)
    SCORE_FORM_ONE = 2,     // score_mfma_all_kernel: one launch over all classes
    SCORE_FORM_SIDE = 3,    // the largest class on the handle's stream, the others on side streams
    SCORE_FORM_SEQ = 4      // one launch per class, one after the other
};
enum ScoreFormMsg { SCORE_MSG_NONE = 0, SCORE_MSG_NO_NETWORK, SCORE_MSG_NO_VARIANT, SCORE_MSG_MEASURE };

static inline const char *score_form_msg(int msg)
{
    switch (msg) {
    case SCORE_MSG_NO_NETWORK: return "no network set for this candidate size";
    case SCORE_MSG_NO_VARIANT: return "score: no histogram variant for this selection mode";
    case SCORE_MSG_MEASURE: return "score: the selection mode ranks by a measure this launch does not compute";
    default: return "";
    }
}

struct ScoreFormIn {
    int variant = SDPCUT_KERNEL_MFMA;      // SDPCUT_OPT_KERNEL
    uint32_t flags = 0;                    // SDPCUT_EIG | SDPCUT_NN
    // per size class (index k = 2 .. SDPCUT_MAX_K): candidates, a network is set, its shape is NetShape<k> (net_shape_is), its
    // pre-activations are bounded (NetDev::unclamped_ok)
    int64_t n[SDPCUT_MAX_K + 1] = {};
    bool net_set[SDPCUT_MAX_K + 1] = {}, shape_ok[SDPCUT_MAX_K + 1] = {}, unclamped_ok[SDPCUT_MAX_K + 1] = {};
    int64_t n_total = 0;                   // candidates of the list
    bool fuse = false;                     // a ScoreFuse was handed in ...
    int fuse_mode = 0;                     // ... for a selection of this TK_MODE_*
    bool eig_kernel = true, one_launch = true;      // SDPCUT_OPT_EIG_KERNEL, SDPCUT_OPT_ONE_LAUNCH
    int side_streams = 0, side_choice = -1;         // SDPCUT_OPT_SIDE_STREAMS; what the list's calibration found (-1: not measured)
    int timing = 0;                        // SDPCUT_OPT_TIMING
};

struct ScoreForm {
    int err = 0;                // 0, or the SDPCUT_E* the call is refused with
    int msg = SCORE_MSG_NONE;   // ScoreFormMsg
    bool fused = false;         // the launches count for the selection (the ScoreFuse is kept)
    int form = SCORE_FORM_SEQ;
    // side_streams == 2 and the list has not been measured: calibrate_side_streams first, then SCORE_FORM_SIDE if it chose the
    // side streams and SCORE_FORM_SEQ (which `form` says) otherwise
    bool calibrate = false;
    bool timed = false;         // the launches carry the handle's two events
    int first = 0, last = 0;    // smallest / largest non-empty size class (0: none)
    int kbig = 0;               // the class with the most candidates (the smallest such size)
    int nclasses = 0;
};

// does size class k run on the MFMA / VALU kernels?  (Without SDPCUT_NN the network part of the kernel is skipped.)
static inline bool score_class_shaped(const ScoreFormIn &in, int k)
{
    return !(in.flags & SDPCUT_NN) || (in.net_set[k] && in.shape_ok[k]);
}

// Everything is decided before anything is launched.  The refusals, with the place each had before this function existed
// (score.hip of commit e7ccc35, where launch_score_k and launch_classes_one made them launch by launch):
//  1. SDPCUT_EINVAL / SCORE_MSG_MEASURE, eigenvalue-only form with a kept fuse whose mode is not TK_MODE_FEAS -- an unsupported
//     mode included: launch_score, :1555.
//  2. SDPCUT_ESTATE / SCORE_MSG_NO_NETWORK, SDPCUT_NN with a non-empty class that has no network: launch_score_k, :1328 (there
//     after the classes in front of it had been launched, and after a calibration).
//  3. SDPCUT_EINVAL / SCORE_MSG_NO_VARIANT, a kept fuse whose mode is none of FEAS / OPT / STRONG: launch_score_k, :1358
//     (launch_classes_one, :1392, only declined such a call and left the refusal to the per-class launches).
//  4. SDPCUT_EINVAL / SCORE_MSG_MEASURE, a kept fuse of mode FEAS without SDPCUT_EIG, or of mode OPT / STRONG without SDPCUT_NN:
//     launch_score_k, :1360 (launch_classes_one, :1393, declined the first of the two).
// 2 excludes 3 and 4 (a fuse is only kept when every class is shaped, which with SDPCUT_NN means it has a network), and none of
// them depends on the class: whichever order the classes were launched in, the first refusal met was this one.
static inline ScoreForm score_form(const ScoreFormIn &in)
{
    ScoreForm f;
    const bool mfma = in.variant == SDPCUT_KERNEL_MFMA;
    bool shaped = true, networks = true, bounded = true;
    for (int k = 2; k <= SDPCUT_MAX_K; ++k) {
        if (in.n[k] <= 0) continue;
        if (!f.first) f.first = k;
        f.last = k;
        ++f.nclasses;
        if (!f.kbig || in.n[k] > in.n[f.kbig]) f.kbig = k;
        shaped = shaped && score_class_shaped(in, k);
        networks = networks && in.net_set[k];
        bounded = bounded && in.net_set[k] && in.unclamped_ok[k];
    }
    // the histograms are built by the MFMA kernels only: every non-empty size class must run on them
    f.fused = in.fuse && mfma && f.nclasses > 0 && shaped;
    const int mode = f.fused ? in.fuse_mode : 0;
    const bool mode_known = mode == 0 || mode == TK_MODE_FEAS || mode == TK_MODE_OPT || mode == TK_MODE_STRONG;
    auto refuse = [&f](int err, int msg) { f.err = err; f.msg = msg; return f; };

    if (in.flags == SDPCUT_EIG && mfma && in.eig_kernel) {      // a pure-feasibility scan has its own kernel
        f.form = SCORE_FORM_EIG;
        f.timed = in.timing != 0 && in.n_total > 0;
        if (f.fused && mode != TK_MODE_FEAS) return refuse(SDPCUT_EINVAL, SCORE_MSG_MEASURE);
        return f;
    }
    f.timed = in.timing != 0 && f.first != 0;
    if ((in.flags & SDPCUT_NN) && !networks) return refuse(SDPCUT_ESTATE, SCORE_MSG_NO_NETWORK);
    if (!mode_known) return refuse(SDPCUT_EINVAL, SCORE_MSG_NO_VARIANT);
    if (mode == TK_MODE_FEAS ? !(in.flags & SDPCUT_EIG) : (mode != 0 && !(in.flags & SDPCUT_NN))) return refuse(SDPCUT_EINVAL, SCORE_MSG_MEASURE);

    // One launch over all classes: every class on the MFMA kernel with the shipped kind of network (pre-activations provably
    // bounded: the clamp-free instantiation, whose scores are what the per-class launches of such networks produce, bit for bit)
    if (f.nclasses > 1 && in.one_launch && mfma && (in.flags & SDPCUT_NN) && shaped && bounded)
        f.form = SCORE_FORM_ONE;
    else if (f.nclasses > 1 && !f.timed && in.side_streams) {
        f.calibrate = in.side_streams == 2 && in.side_choice < 0;
        f.form = (in.side_streams == 1 || in.side_choice == 1) ? SCORE_FORM_SIDE : SCORE_FORM_SEQ;
    }
    return f;
}
