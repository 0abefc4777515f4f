// Internal to the scoring: what the score kernels are handed (ScoreArgs), the one place it is filled, and the launchers through
// which score.hip (host only) starts the kernels of score_mfma.hip and score_alt.hip.  No kernel is referenced from another
// translation unit.  Grids and the work split come from the plan (score_plan.h); the launchers enqueue and leave
// hipGetLastError to the caller.
#pragma once
#include <hip/hip_ext.h>

#include "common.h"
#include "score_plan.h"
#include "topk_dev.h"

struct ScoreArgs {
    const int32_t *set;   // SoA [K][n]
    const int32_t *orig;  // [n]
    int64_t n;
    // score_mfma_kernel: candidates per strip of a wave, 64 or 32 (score_plan; see the kernel)
    int32_t strip;
    // Balanced tail round (r4, score_plan): candidates [0, rr_end) go round-robin in whole strips as before; the rest --
    // less than one strip per wave -- is split EVENLY: wave g takes tail_hi (g < tail_nhi) or tail_lo column tiles of 16
    // candidates from rr_end on.  rr_end = n, tail_hi = tail_lo = 0: no tail (every list but the ones the rule in score_plan.h picks).
    int64_t rr_end;
    int64_t tail_nhi;
    int32_t tail_hi, tail_lo;
    const double *vars;   // [L + nv]: X packed | x
    const double *Q;      // [L]
    int32_t nv;
    int64_t L;
    double *eig_out;      // [N] caller order
    double *obj_out;      // [N]
    uint32_t flags;
    // Leading-digit histogram of the top-k selection that follows (topk_dev.h; tk == nullptr: off): the
    // kernel that produces the scores also counts the members of the selection's class by the first radix
    // digit of their keys -- in LDS per workgroup, flushed with no-return atomics at its end (no ticket,
    // nobody waits) -- together with the violated / positive counters.  The selection then starts at its
    // second digit and builds the keys from the scores as it reads them: the separate key pass
    // (tk_keys_kernel, 17.5 us per round) is gone.  Candidates outside the class (key 0) are not counted:
    // the selection never looks below the class.
    TopkWs *tk;
    int tk_mode;           // TK_MODE_FEAS / OPT / STRONG: the kernel's FUSE template argument
    int32_t spread;        // the four waves of a workgroup take strips from four distant quarters of the list (see score_mfma_body)
    int32_t pf_mloc;       // fine histogram of the class (topk_dev.h): a workgroup reports its table down to its pf_mloc-th largest member; 0: off
    // optional: += number of candidates with obj_improve > 0 and lambda_min < -1e-15 (the "strong" class
    // of the combined strategy, cut_select_qp.py:607-613); lets the selection that follows pick its
    // regime on the device.  Needs both flags.
    int64_t *strong_out;
    // SKIP / FILTER kernels, optional (NULL: off): every candidate the launch finds strong is appended to this list -- its selection
    // key into emit[2 slot], its output index into emit[2 slot + 1], slot from one returning atomic per pass on tk->emit_n; entries
    // beyond emit_cap are dropped and raise tk->emit_over.  Append order is not deterministic.
    uint64_t *emit;
    uint32_t emit_cap;
    NetDev net;
};

// the launch over all size classes of a list (score_mfma_all_kernel, score_mfma.hip)
struct ScoreArgsAll {
    ScoreArgs a[SDPCUT_MAX_K - 1];      // classes in launch order
    int32_t k[SDPCUT_MAX_K - 1];        // their sizes
    int32_t bend[SDPCUT_MAX_K - 1];     // one past their last workgroup
    int32_t nclasses;
};

// What a launch over the handle's class K passes to its kernel; the work split is the plan's (score_plan).
static inline ScoreArgs fill_score_args(const sdpcut_ctx *h, int K, uint32_t flags, const ScoreFuse *fuse, int64_t *strong_out,
                                        const ScorePlan &p)
{
    const Bucket &b = h->bucket[K];
    ScoreArgs A;
    A.set = b.d_set.get(); A.orig = b.d_orig.get(); A.n = b.n;
    A.strip = p.strip;
    A.rr_end = p.rr_end; A.tail_nhi = p.tail_nhi; A.tail_hi = p.tail_hi; A.tail_lo = p.tail_lo;
    A.vars = score_vars(h, flags); A.Q = score_Q(h, flags); A.nv = h->nb_vars; A.L = h->L;      // (a node box: common.h)
    A.eig_out = h->d_eig.get(); A.obj_out = h->d_obj; A.flags = flags;
    A.tk = fuse ? (TopkWs *)fuse->ws : nullptr;
    A.tk_mode = fuse ? fuse->mode : 0;
    A.spread = p.spread;
    A.pf_mloc = p.pf_mloc;
    A.strong_out = ((flags & SDPCUT_EIG) && (flags & SDPCUT_NN)) ? strong_out : nullptr;
    A.emit = nullptr; A.emit_cap = 0;      // (set by the launch that skips: launch_score_k)
    A.net = h->net[K].dev;
    return A;
}

// A batch of LP points (points.hip): what workgroup row y of score_mfma_points_kernel adds to the pointers of its ScoreArgs, in
// elements: vars += y * vars, eig_out / obj_out += y * scores, strong_out (if set) += y * strong, Q += y * Q (0: one Q for all
// points; L: every point has a Q' of its own, a boxed batch).
struct ScorePointStrides {
    int64_t vars, scores, strong, Q;
};

// With SDPCUT_OPT_TIMING the kernel's own dispatch carries the two events (hipExtLaunchKernelGGL):
// its start / end timestamps are taken from the dispatch packet, without the two barrier packets
// and ~20 us per step that hipEventRecord around the launch costs.
#define SCORE_LAUNCH(kern, grid, block)                                                              \
    do {                                                                                             \
        if (ev_start || ev_stop)                                                                     \
            hipExtLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, st, ev_start, ev_stop, 0, A);       \
        else                                                                                         \
            hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, st, A);                             \
    } while (0)

// score_mfma.hip.  The FUSE argument of the kernel is A.tk_mode where A.tk is set (one of TK_MODE_FEAS / OPT / STRONG: score_form
// has refused everything else) and 0 otherwise.
void score_mfma_launch(int K, const ScoreArgs &A, int grid, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop);   // score_mfma_kernel, CLAMP = !A.net.unclamped_ok
// score_mfma_skip_kernel (the MLP for violated candidates only) over class K, if score_mfma_skip_built(K): A.tk set, A.tk_mode
// TK_MODE_STRONG, both flags, the work split of score_plan_skip
bool score_mfma_skip_built(int K);
void score_mfma_skip_launch(int K, const ScoreArgs &A, int grid, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop);
// score_mfma_filter_kernel (the skipping kernel with the fp32 filter in front of the fp64 pass) over class K, if
// score_mfma_filter_built(K) and A.net.filter_ok: the arguments and the work split of score_mfma_skip_launch
bool score_mfma_filter_built(int K);
void score_mfma_filter_launch(int K, const ScoreArgs &A, int grid, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop);
// filter_audit_kernel: the filter's fp32 pass for every candidate of class K, unmapped outputs into d_y32 [N] and, if d_m is not
// null, the candidates' margins into d_m [N] (caller order)
void score_filter_audit_launch(int K, const ScoreArgs &A, int grid, double *d_y32, double *d_m, hipStream_t st);
void score_mfma_all_launch(const ScoreArgsAll &AA, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop);            // score_mfma_all_kernel over AA.bend[nclasses - 1] workgroups
// score_mfma_points_kernel over class K at n_points points: grid x n_points workgroups, A.tk must be NULL
void score_mfma_points_launch(int K, const ScoreArgs &A, const ScorePointStrides &ps, int grid, int n_points, hipStream_t st);
// score_alt.hip: score_valu_kernel (valu; the class's network has the shape of NetShape<K>) or score_simple_kernel
void score_alt_launch(int K, bool valu, const ScoreArgs &A, int n_cu, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop);
