/*
 * sdpcut.h -- C-ABI of the MI355X (gfx950) cut-scoring library  libsdpcut_hip.so
 *
 * Drop-in boundary for ONE hot path of rb2309/SDPCutSel-via-NN: the per-round scoring,
 * ranking and generation of low-dimensional PSD cuts.  The reference reaches native code
 * for this path through exactly one FFI:
 *
 *     ctypes.cdll.LoadLibrary('neural_nets/NNs.so')            cut_select_qp.py:297
 *     double neural_net_{2,3,4,5}D(const double X[d(d+3)/2])   cut_select_qp.py:299-303, 579-582
 *
 * i.e. one scalar MLP evaluation per candidate per call, with the gather, the eigen-
 * decomposition (numpy/LAPACK, cut_select_qp.py:788-797), the scoring arithmetic
 * (:573-582), the ranking (:601-654) and the cut rows (:737-750) done in Python around it.
 * This library replaces that per-candidate FFI by a batched, handle-based one that runs
 * the whole per-round computation on the GPU.  Each entry point below names the reference
 * lines it replaces.  Plain C types only: caller-owned contiguous host buffers unless a
 * parameter is named d_* (device pointer).  Every function returns 0 on success or a
 * negative SDPCUT_E* code; sdpcut_last_error() returns the message.  A handle is not
 * re-entrant; different handles are independent (one per GPU / per thread).
 *
 * There is NO CPU fallback: every entry point needs a gfx950 device and fails with
 * SDPCUT_ENODEVICE otherwise.
 */
#ifndef SDPCUT_H
#define SDPCUT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: what this header declares is ALL it exports (tests/test_host_cpu.py) */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

typedef struct sdpcut_ctx *sdpcut_handle;

enum {
    SDPCUT_OK = 0,
    SDPCUT_EINVAL = -1,    /* bad argument (mirrors the reference's asserts, cut_select_qp.py:91-94) */
    SDPCUT_ENODEVICE = -2, /* no usable gfx950 device */
    SDPCUT_EHIP = -3,      /* HIP runtime error */
    SDPCUT_ESTATE = -4,    /* call order violated (e.g. score before set_point) */
    SDPCUT_ENOMEM = -5
};

/* score flags (SDPCUT_SDP: the exact optimum of the small SDP the MLP of SDPCUT_NN estimates; SDPCUT_EFF: the efficacy of the cut
 * row a round would emit; see sdpcut_score) */
enum { SDPCUT_EIG = 1, SDPCUT_NN = 2, SDPCUT_SDP = 4, SDPCUT_EFF = 8 };

/* selection strategies, numbering of cut_select_algo (cut_select_qp.py:79-80); SDPCUT_STRAT_EXACT is accepted only while
 * SDPCUT_OPT_EXACT_SDP is on */
enum { SDPCUT_STRAT_FEAS = 1, SDPCUT_STRAT_OPT = 2, SDPCUT_STRAT_EXACT = 3, SDPCUT_STRAT_COMB = 4 };
/* Strategy 6, efficacy: all N candidates by the score of SDPCUT_EFF descending (the first criterion of a MIP solver's cut selector,
 * optionally plus w times the objective parallelism), ties by ascending candidate index -- strategy 2's semantics on another array:
 * n_total = N, *new_strat = 6, nb_positive counts escore > 0 (= nb_violated).  Not a strategy of the reference (its numbering ends
 * at 5).  Accepted by sdpcut_rank / sdpcut_rank_device (which need a preceding sdpcut_score(SDPCUT_EFF); sdpcut_rank_fetch after
 * them), sdpcut_select_round, sdpcut_select_round_view, sdpcut_round_view, sdpcut_round_csr, sdpcut_round_csr_begin / _end,
 * sdpcut_round_csr_diverse and sdpcut_round_csr_multi: the fused calls score the measure themselves if it is missing, then run
 * the selection strategy 2 runs on scores that exist already; `score` of every head is escore, and the rows are computed from the
 * lambda_min the score was computed from.  No networks needed.  SDPCUT_OPT_EXACT_HEAD ignores it.  Refused with SDPCUT_EINVAL: by
 * the plain batched-points calls (sdpcut_score_points, sdpcut_round_csr_points and their _boxed forms; over many LP points the
 * measure and the strategy come through sdpcut_efficacy_points and sdpcut_round_csr_points_diverse) and the sharded entry points
 * (sdpcut_shard_*). */
enum { SDPCUT_STRAT_EFF = 6 };
/* Partial ranking for candidate sets sharded over several GPUs (SURVEY.md section 8 e): only
 * the "strong" class of the combined scan (cut_select_qp.py:607-613: obj_improve > 0 and
 * violated), by obj_improve.  Its merged per-shard heads give the global position at which
 * the reference's scan stops.  n_total / counters[0] = size of the class. */
enum { SDPCUT_PART_STRONG = 104 };
/* The other regime of the combined scan over shards: fewer than sel_size strong candidates exist OVERALL, so the scan
 * visits every entry (cut_select_qp.py:606-623) and each shard's own combined ranking is a sub-list of the global one.
 * sdpcut_shard_head_device with this value packs the shard's head by (new score, obj_improve, id) with obj_improve as a
 * third field of the record (the merge's secondary key: the second stable sort of :625 keeps the order of the first, :601). */
enum { SDPCUT_PART_COMBALL = 105 };

/* kernel variants for sdpcut_set_option(SDPCUT_OPT_KERNEL, ...).  The variants agree on the optimality measure to rounding, not to
 * the bit: CHANGING the variant invalidates the optimality scores of the current list at the current point, as replacing a network
 * does (the next call that needs them computes them again; lambda_min and the exact measure are kept), and is refused with
 * SDPCUT_ESTATE while a round is pending. */
enum { SDPCUT_KERNEL_MFMA = 0, SDPCUT_KERNEL_SIMPLE = 1, SDPCUT_KERNEL_VALU = 2 };
/* SDPCUT_OPT_FUSE_KEYS (default 1): sdpcut_select_round lets the score kernels count their scores by
 * the leading radix digit of the selection keys (per workgroup in LDS, flushed with no-return atomics)
 * together with the violated / positive counters; the top-k selection then starts at its second digit
 * and builds the keys from the scores while it reads them, so the separate key pass over the scores
 * (17.5 us per round at 10^6 candidates) disappears.  0: the selection runs its own first pass. */
/* SDPCUT_OPT_AUTO_REGIME (default 1): sdpcut_select_round with the combined strategy lets the score
 * kernels count the strong candidates and the selection pick its regime on the device (one selection,
 * no host round trip whether or not sel_size strong candidates exist).  0: the selection assumes the
 * common regime and the host repeats it when the count says otherwise (the round-1 behaviour). */
/* SDPCUT_OPT_FUSED_TAIL (default 1): the top-k selection runs its later passes, the count and the
 * compaction in one launch behind bounded grid barriers instead of four launches; 0 = one launch per
 * pass (A/B and fallback). */
/* SDPCUT_OPT_COOP_LAUNCH (default 0): make that launch a cooperative one (hipLaunchCooperativeKernel), so
 * that the runtime guarantees the co-residency its grid barriers rely on.  Measured on MI355X: +20 us per
 * round (0.455 instead of 0.435 ms).  Without it the grid is capped at one workgroup per CU (256 x 256
 * threads, 38 KB of LDS each), which an otherwise idle device always holds, and every wait is bounded: a
 * barrier that does not complete within a few milliseconds voids the selection and the full-sort path
 * answers (counted by SDPCUT_STAT_SELECT_FALLBACKS). */
/* SDPCUT_OPT_EIG_KERNEL (default 1): launches that compute only lambda_min (feasibility rounds,
 * cut_select_qp.py:639-654) run the dedicated eigenvalue kernel -- one launch over all size classes, compiled
 * without the MLP's register state -- instead of the scoring kernels' eigenvalue branch (0: A/B). */
/* SDPCUT_OPT_ONE_LAUNCH (default 1): a list with several size classes is scored by ONE launch in which every class has its own
 * range of workgroups (the shipped networks; same scores bit for bit as a launch per class).  0, or a list the launch does not
 * cover (user networks that need the clamped path, the VALU / simple kernel variants): a launch per class, see the next option. */
/* SDPCUT_OPT_SIDE_STREAMS (default 0 since r4 -- the default configuration picks no code path from a timing; only lists that
 * SDPCUT_OPT_ONE_LAUNCH does not cover get here at all): a list with several size classes may score its smaller classes on side streams of the handle,
 * between a fork and a join event, next to the largest class on the handle's stream.  0: one launch after the other; 1: side
 * streams; 2: the first multi-class scoring of a candidate list measures both forms (~1 ms, once) and keeps the faster --
 * whether the streams run side by side depends on which hardware queues the process's streams were given. */
/* SDPCUT_OPT_STREAM_PRIORITY (default 0): 1 re-creates the handle's own stream with the device's highest priority.  For a handle
 * whose list is SHORT and whose rounds run next to another handle's (the QCQP round's objective cover beside its constraints
 * cover, sdpcut_round_csr_begin): its few small kernels are then dispatched ahead of the other list's waiting workgroups instead of
 * behind them.  Not allowed while a round is pending; ignored by a handle that runs on a caller's stream (sdpcut_set_stream). */
/* SDPCUT_OPT_PREFILTER (default 1; needs SDPCUT_OPT_FUSE_KEYS): the eigenvalue kernel (every class) and the score kernel (3-variable
 * classes) of a fused round also count the class members in a 2048-bin window over the top seventeen bits of their selection keys
 * (csrc/topk_dev.h: one LDS atomic per candidate; a workgroup reports, when it retires, only the bins down to the one that holds
 * its own m-th largest member, and publishes that floor).  Where the bin of the k-th largest key lies above every floor and its
 * members fit the sort buffers, the selection is resolved from the table: one pass over the scores, no digit pass, no grid barrier.
 * 0: the radix passes of rounds 2-4 (A/B; identical results). */
/* SDPCUT_OPT_EXACT_HEAD (default 0): the head a selection under strategy 2 or 4 returns is the head of the reference's ranking
 * with obj_improve computed in the REFERENCE's operation order (the arithmetic of SDPCUT_KERNEL_SIMPLE: no contraction, the host
 * libm's exp, sums in index order) and this library's lambda_min; `score` carries those bits (strong class: the fp64 sum with
 * BIG_M, cut_select_qp.py:611; entries whose score is -lambda_min are untouched), ties between equal exact scores go by ascending
 * candidate index, the cut rows are those of that head, and under strategy 4 the classes, n_total / new_strat / counters follow
 * the exact signs (strategy 2 has no class: its counters are what the option-off call reports).  The fast
 * (MFMA) scores only filter: the selection runs for min(N, cap + max(256, cap / 8)) entries, that band is re-scored and
 * re-ranked on the device, and csrc/exact_band.h decides on the device whether the band provably holds the exact head (the fast
 * scores are within 1e-9 max(|obj|, 1e-3 max_elem) of the exact ones; measured 2e-11).  A band that does not is retried once with
 * 8192 entries; if that fails too (masses of equal scores at the threshold; more than 1024 candidates whose sign the fast score
 * cannot decide) the call GIVES UP: it returns exactly what it returns with the option off -- never a half-exact head -- and
 * SDPCUT_STAT_EXACT_GAVE_UP counts it.  A band selection that is void because one of its bounded waits expired is neither exact
 * nor a reason to retry with the widest band: the call gives up in the same way (SDPCUT_STAT_EXACT_GAVE_UP + 1,
 * SDPCUT_STAT_EXACT_HEAD = 0, SDPCUT_STAT_SELECT_FALLBACKS unchanged) and the round is the option-off round, bit for bit.
 * Affects sdpcut_select_round*, sdpcut_round_view, sdpcut_round_csr*, and sdpcut_rank / sdpcut_rank_device when the head asked for
 * is within the limit below (strategy 4: and max_out <= sel_size); strategies 1 and SDPCUT_PART_* ignore it.
 * Head limit: min(N, cap + max(256, cap / 8)) <= 8192 (the reference's cap is 5000); a fused round with a longer head fails with
 * SDPCUT_EINVAL while the option is on, sdpcut_rank* beyond it rank as with the option off.  The sharded entry points
 * (sdpcut_shard_*) fail with SDPCUT_ESTATE while it is on.
 * d_obj is NOT written back: sdpcut_get_scores and sdpcut_gather_scores_device keep returning what the score kernel produced. */
/* SDPCUT_OPT_EXACT_SDP (default 0): strategy 3 of cut_select_algo -- optimality via the EXACT SDP solution, cut_select_qp.py:584-598
 * -- is accepted by sdpcut_rank / sdpcut_rank_device (and sdpcut_rank_fetch after them), sdpcut_select_round, sdpcut_select_round_view,
 * sdpcut_round_view, sdpcut_round_csr and sdpcut_round_csr_begin / _end.  It is strategy 2 with the exact measure of SDPCUT_SDP in
 * place of the MLP's estimate: all N candidates by that measure descending, ties by ascending candidate index (:601); n_total,
 * counters as under strategy 2 (nb_positive counts the exact measure), *new_strat = 3.  sdpcut_rank* need a preceding
 * sdpcut_score(SDPCUT_SDP); the fused calls score it themselves if it is missing, then run the selection that strategy 2 runs on
 * scores that exist already.  No networks needed.  SDPCUT_OPT_EXACT_HEAD ignores strategy 3; the sharded entry points
 * (sdpcut_shard_*) refuse it.  With the option off strategy 3 is refused exactly as before (SDPCUT_EINVAL, "strategy must be ..."). */
/* SDPCUT_OPT_COUNT_RANK (default 1): the sort tail of a top-k selection whose head fits 8192 entries orders the compacted
 * superset of the head by COUNTING in one launch (csrc/topk_sort.hip, tk_countrank_kernel: the rank of an entry is the number of
 * (key, [obj_improve,] index) composites in front of it) instead of a tile sort and a rank merge in two.  Same head, bit for bit.
 * 0: the two launches (A/B; they also serve heads of 8193 .. 16384 entries, raw key output and shard records either way). */
/* SDPCUT_OPT_SKIP_NONVIOLATED (default 1): a fused combined round (sdpcut_select_round*, sdpcut_round_*, sdpcut_shard_head_device with
 * SDPCUT_PART_STRONG) whose list holds one size class with a skipping kernel (3-variable candidates; csrc/score_plan.h:
 * SDPCUT_SKIP_KMASK) runs the MLP only for VIOLATED candidates: in its strong regime -- at least sel_size candidates violated with a
 * positive measure -- the ranking of cut_select_qp.py:601-632 reads the measure of no other.  Same head, scores, rows, new_strat,
 * nb_violated / strong / violated_in_scan, bit for bit; nb_positive of such a round counts the positive measures among the
 * VIOLATED candidates (the others were not evaluated).  A round that turns out to visit every entry completes the measure (one
 * NN-only scoring launch) and runs again inside the call; so does whatever else reads the measure of the list afterwards
 * (sdpcut_get_scores, sdpcut_rank*, sdpcut_gather_scores_device, diverse / multi-cut / pool rounds, strategy 2):
 * SDPCUT_STAT_NN_COMPLETIONS counts those launches, SDPCUT_STAT_SCORED reports SDPCUT_NN either way.
 * 1: lists the score kernel cuts into strips of 64 (more than 65 536 candidates on a 256-CU device); 0: never; 2: every list (tests). */
/* SDPCUT_OPT_FP32_FILTER (default 1): where a launch under SDPCUT_OPT_SKIP_NONVIOLATED runs and the class's network qualifies
 * (sdpcut_get_filter_margin), the violated candidates first go through the network in fp32 on the matrix cores; the fp64 pass
 * then runs only for those whose fp32 measure exceeds -margin * max_elem, margin a PROVEN bound on the difference of the two network
 * outputs (csrc/net_pack.h), and for candidates with an input outside the domain the bound was derived on.  The margin is PER
 * CANDIDATE -- it follows the slopes of the last hidden layer's activations at that candidate -- and never above
 * sdpcut_get_filter_margin (sdpcut_filter_audit_margins returns it).  Every violated
 * candidate with a positive measure is among them: same head, scores, rows, new_strat and counters as with the option off, bit for
 * bit; the others keep their fp32 measure, which is not positive, until the measure is completed on demand exactly as under
 * SDPCUT_OPT_SKIP_NONVIOLATED (no call returns it before).
 * 0: never filter. */
enum { SDPCUT_OPT_KERNEL = 1, SDPCUT_OPT_TIMING = 2, SDPCUT_OPT_FUSE_KEYS = 3, SDPCUT_OPT_AUTO_REGIME = 4,
       SDPCUT_OPT_FUSED_TAIL = 5, SDPCUT_OPT_COOP_LAUNCH = 6, SDPCUT_OPT_EIG_KERNEL = 7, SDPCUT_OPT_STREAM_PRIORITY = 8,
       SDPCUT_OPT_SIDE_STREAMS = 9, SDPCUT_OPT_ONE_LAUNCH = 10, SDPCUT_OPT_PREFILTER = 11, SDPCUT_OPT_EXACT_HEAD = 12, SDPCUT_OPT_EXACT_SDP = 13,
       SDPCUT_OPT_COUNT_RANK = 14, SDPCUT_OPT_SKIP_NONVIOLATED = 15, SDPCUT_OPT_FP32_FILTER = 16, SDPCUT_OPT_INJECT_GIVEUP = 17 };
/* SDPCUT_OPT_INJECT_GIVEUP (default 0) -- TEST ONLY.  Makes the bounded device waits of the library give up without waiting, so that
 * the recovery paths behind them can be tested on an idle device.  value = SDPCUT_INJECT_GIVEUP(site, first, count):
 *   site   1 the top-k selection of more than one workgroup (the fused kernel with its grid barriers and its wait for a published
 *            digit, and the launch-per-digit route that stands in for it, which the hook hits in the same way),
 *          2 the look-back of the ordered CSR row assembly (plain, multi-cut, diverse and batched-points rounds);
 *   first  0 .. 255 launches of that site pass untouched, then
 *   count  1 .. 255 launches of that site are hit.
 * The option disarms itself with the last hit; 0 disarms it by hand.  SDPCUT_ESTATE while a round is pending.
 * A hit selection ends with its void mark raised (as after an expired wait: workgroups that reach a wait leave, the head of the
 * others is discarded) and the host answers through its path without waits.  In a hit assembly launch every workgroup behind the
 * first gives up its look-back before the first poll, whether or not the word it would wait for has arrived; the host launches
 * the assembly again and fails with SDPCUT_EHIP after the second give-up.  Launches without a bounded wait are no site and consume
 * nothing: the one-workgroup selections (lists of a few thousand candidates, the batched points), an assembly of one workgroup (a
 * head of <= 64 entries).
 * The hook never waits, never spins and launches nothing of its own.  With the option at 0 every call does what it did before. */
#define SDPCUT_INJECT_GIVEUP(site, first, count) (((int64_t)(site) << 16) | ((int64_t)(first) << 8) | (int64_t)(count))
/* SDPCUT_OPT_EMIT_HEAD (default 1): the scoring launch of a fused combined round under SDPCUT_OPT_SKIP_NONVIOLATED also appends every
 * candidate it finds strong -- its selection key and its index -- to a list in the selection's workspace, and a round that resolves
 * to its strong regime selects its head from that list instead of rebuilding the key of every candidate from the score arrays
 * (csrc/topk_route.h: TK_ROUTE_EMITTED).  Same head, scores, rows, counters and new_strat, bit for bit; a round in the other regime,
 * or one whose list overflowed, scans the scores as with the option off.  0: nothing is appended, the selection is the one of
 * TK_ROUTE_ONFLY (A/B, tests).  SDPCUT_ESTATE while a round is pending.
 * SDPCUT_OPT_EMIT_CAP (default 0) -- TEST ONLY: > 0 caps the list at that many entries, so that the overflow path can be run on a
 * short list; 0: the capacity the workspace gives (half the list length). */
#define SDPCUT_OPT_EMIT_HEAD 18
#define SDPCUT_OPT_EMIT_CAP 19

/* Counters of a handle: SDPCUT_STAT_ROUNDS = fused rounds served (sdpcut_select_round*),
 * SDPCUT_STAT_SELECT_FALLBACKS = rounds whose radix selection declared itself void (a grid barrier
 * timed out because other work kept its workgroups from starting) and were answered by the full-sort
 * path instead -- same result, ~1 ms instead of ~0.1 ms; also: skipped rounds begun again for that reason, sdpcut_tri_separate
 * calls that ran their selection once more, and row assemblies launched once more because their look-back gave up (one per
 * launch; per point in the batched rounds).  The table is DESIGN.md section 5 "Give-up paths".
 * SDPCUT_STAT_SCORED = the measures (SDPCUT_EIG | SDPCUT_NN | SDPCUT_SDP | SDPCUT_EFF) scored at the current point.
 * SDPCUT_STAT_TIE_SPLITS (r4) = every-entry-visited combined rankings whose threshold group of EQUAL new scores
 * did not fit the sort buffers (structured LP vertices) and was cut by its secondary key -- obj_improve, then index,
 * cut_select_qp.py:601 under :625 -- with two more radix selections; until round 3 these rounds were fallbacks.
 * SDPCUT_STAT_DIRECT_SELECTIONS (r5) = selections resolved from the fine histogram the score kernels leave (no digit pass, no grid
 *   barrier: SDPCUT_OPT_PREFILTER); the others ran the radix passes (short lists, masses of equal keys at the threshold, the
 *   every-entry-visited regime).  Read from the device: the call waits for the handle's stream.  Same results either way.
 * SDPCUT_STAT_PF_BIN / _PF_FLOOR / _PF_COUNT: what the last selection that looked at the fine histogram found there -- the fine bin of
 *   the k-th largest key (-1: none), the floor the producers published (fine bins), the members at or above that bin.  Diagnostics.
 * SDPCUT_STAT_EXACT_HEAD = 1 if the last selection returned an exact head (SDPCUT_OPT_EXACT_HEAD), else 0;
 * SDPCUT_STAT_EXACT_GAVE_UP = selections under the option that returned the ordinary head because a band did not fit;
 * SDPCUT_STAT_EXACT_RETRIES = selections whose first band did not prove itself and that ran again with the widest one.
 * SDPCUT_STAT_SDP_UNCONVERGED = candidates of the last exact-SDP solve (sdpcut_score with SDPCUT_SDP, or sdpcut_sdp_batch) that stopped
 *   at the iteration cap instead of the gap target; they still returned their certified lower bound and their gap.  Read from the
 *   device: the call waits for the handle's stream.
 * SDPCUT_STAT_POINTS_REDONE = points of batched rounds (sdpcut_round_csr_points) on the one-launch route whose selection declared
 *   itself void -- an every-entry-visited tie group beyond the one-workgroup sort, a structured LP vertex -- and that were served
 *   by the single-point round inside the call instead.  Same results either way.
 * SDPCUT_STAT_NN_SKIPPED = candidates the handle's last scoring launch did not run the MLP for: list length - nb_violated after a
 *   launch under SDPCUT_OPT_SKIP_NONVIOLATED, 0 after any other (a completion included) and after a new list; after
 *   sdpcut_shard_head_device it is read from the device: the call waits for the handle's stream;
 * SDPCUT_STAT_NN_COMPLETIONS = NN scoring launches since the handle was made that completed a measure such a launch left partial.
 * SDPCUT_STAT_NN_EVALUATED = fp64 MLP evaluations of the handle's last scoring launch that ran the network: the list length after a
 *   launch that scored everybody, nb_violated after a skipping launch, the survivors of the fp32 filter after a filtering one --
 *   the violated candidates whose fp32 measure exceeds -margin * max_elem with their OWN margin, which is never above
 *   sdpcut_get_filter_margin -- (read from the device: the call waits for the handle's stream); 0 after a new list.
 * SDPCUT_STAT_DIVERSE_POINTS_FAST = points of sdpcut_round_csr_points_diverse answered by its one-wait route since the handle was made
 *   (points served by the loop inside the call, or redone, do not count).
 * SDPCUT_STAT_INJECTED -- TEST ONLY: launches SDPCUT_OPT_INJECT_GIVEUP has hit since the handle was made.
 * SDPCUT_STAT_TRI_POINTS_FAST = points of sdpcut_tri_round_csr_points answered by its one-wait route since the handle was made
 *   (points served by the loop inside the call do not count). */
enum { SDPCUT_STAT_ROUNDS = 1, SDPCUT_STAT_SELECT_FALLBACKS = 2, SDPCUT_STAT_SCORED = 3, SDPCUT_STAT_TIE_SPLITS = 4,
       SDPCUT_STAT_DIRECT_SELECTIONS = 5, SDPCUT_STAT_PF_BIN = 6, SDPCUT_STAT_PF_FLOOR = 7, SDPCUT_STAT_PF_COUNT = 8,
       SDPCUT_STAT_EXACT_HEAD = 9, SDPCUT_STAT_EXACT_GAVE_UP = 10, SDPCUT_STAT_EXACT_RETRIES = 11,
       SDPCUT_STAT_SDP_UNCONVERGED = 12, SDPCUT_STAT_POINTS_REDONE = 13,
       SDPCUT_STAT_NN_SKIPPED = 14, SDPCUT_STAT_NN_COMPLETIONS = 15, SDPCUT_STAT_NN_EVALUATED = 16,
       SDPCUT_STAT_DIVERSE_POINTS_FAST = 17, SDPCUT_STAT_INJECTED = 18 };
/* (a macro, not an enumerator: the enumeration above is the closed set of codes 1 .. 18 that tests/test_diverse_points_cpu.py pins) */
#define SDPCUT_STAT_TRI_POINTS_FAST 19
/* SDPCUT_STAT_EMITTED_SELECTIONS = selections since the handle was made whose head came from the list the scoring launch emitted
 * (SDPCUT_OPT_EMIT_HEAD; TK_ROUTE_EMITTED in its strong regime without an overflow).  Read from the device: the call waits for the
 * handle's stream. */
#define SDPCUT_STAT_EMITTED_SELECTIONS 20
/* SDPCUT_STAT_NODE_EVAL_POINTS = points evaluated by sdpcut_node_eval_points since the handle was made. */
#define SDPCUT_STAT_NODE_EVAL_POINTS 21
int sdpcut_get_stat(sdpcut_handle h, int which, int64_t *value);

/* The fp32 filter (SDPCUT_OPT_FP32_FILTER) of the network set for k-variable candidates: *margin = the proven bound on
 * |y32 - y64| of the unmapped network output that holds for every candidate -- the filter decides by a margin per candidate that
 * is never above it (sdpcut_filter_audit_margins) --, or NaN if that network does not filter (not clamp-free, not
 * the shipped 3-variable shape, or a bound above the cut-off).  SDPCUT_ESTATE without a network for k. */
int sdpcut_get_filter_margin(sdpcut_handle h, int k, double *margin);
/* Audit of that bound on the device: runs the filter's fp32 pass -- the device function the scoring kernel runs -- for EVERY
 * candidate of the handle's list at the current point and returns the fp32 network output, unmapped, in y32_out [N] (caller
 * order).  The list must hold 3-variable candidates only and their network must filter; no node box.  Not a hot path. */
int sdpcut_filter_audit(sdpcut_handle h, double *y32_out);
/* The same audit, and in m_out [N] (caller order) the margin the filter decides by for each candidate: a proven bound on
 * |y32 - y64| of THAT candidate, computed by the same device function from the same pass, <= sdpcut_get_filter_margin. */
int sdpcut_filter_audit_margins(sdpcut_handle h, double *y32_out, double *m_out);

/* Maximum sub-problem size (assert dim <= 5, cut_select_qp.py:93) */
#define SDPCUT_MAX_K 5
/* row stride of the padded coefficient output of sdpcut_cut_rows: k + k(k+1)/2 <= 20 */
#define SDPCUT_ROW_LD 20

int sdpcut_version(void);
const char *sdpcut_last_error(sdpcut_handle h); /* h may be NULL: error of the last failed create */

/* Lifetime.  Replaces _load_neural_nets' LoadLibrary (cut_select_qp.py:284-303). */
int sdpcut_create(int device_id, sdpcut_handle *out);
int sdpcut_destroy(sdpcut_handle h);
int sdpcut_set_option(sdpcut_handle h, int option, int64_t value);
/* Run all work of this handle on an existing HIP stream (hipStream_t passed as void*).
 * NULL is the HIP null stream (what PyTorch calls its default stream);
 * SDPCUT_OWN_STREAM restores the handle's own non-blocking stream.
 * Order: every launch, copy and event of the library goes to the handle's stream, and device pointers passed to it
 * (d_vars_values, d_idx_out, d_record, d_allrec, ...) are read and written in that stream's order: produce them on the stream,
 * consume them on it, and no host synchronisation is needed.  A switch to ANOTHER stream orders the new stream, on the device,
 * behind everything the handle has enqueued on the old one; the caller need not synchronise first, and the call does not wait on
 * the host (except for a staged sdpcut_set_point transfer still in flight, whose source is host memory).  That matters after the
 * entry points that return without a host wait: sdpcut_score, sdpcut_set_point, sdpcut_set_point_device, sdpcut_wake,
 * sdpcut_round_csr_begin, sdpcut_merge_topk_device, sdpcut_gather_scores_device, sdpcut_shard_head_device and
 * sdpcut_shard_finish_enqueue (sdpcut_set_box and sdpcut_rank_device wait first and leave only their last launches behind).
 * With the stream the handle already has the call changes nothing.
 * Lifetime: the stream stays the caller's.  It must outlive its use by the handle -- until a later sdpcut_set_stream has moved
 * the handle off it (that call still records an event on it) or sdpcut_destroy. */
#define SDPCUT_OWN_STREAM ((void *)(intptr_t)-1)
int sdpcut_set_stream(sdpcut_handle h, void *hip_stream);
int sdpcut_synchronize(sdpcut_handle h);
/* (r5) Enqueue an empty kernel on the handle's stream and return at once.  In the reference's loop a separation round follows an LP
 * solve of 0.1-10 s (cut_select_qp.py:149-200, :193-200) during which the device falls idle; a round issued to an idle device costs
 * 0.1-0.2 ms more than one issued back to back (bench.py: secondary.cold_round).  A caller that pokes the device as soon as its
 * solver returns -- before it extracts the solution vector -- gets 40-65 us of that back.  Optional; changes no result. */
int sdpcut_wake(sdpcut_handle h);

/*
 * Trained MLP for k-variable candidates (replaces the constants baked into NNs.so;
 * neural_nets/neural_net_kD.m constants section).  n_layers counts the linear output
 * layer; widths[l] = outputs of layer l (last = 1).  params is packed as
 *   xoffset[d_in], gain[d_in], ymin,
 *   for each layer: W[width][fan_in] row-major, b[width],
 *   y_ymin, y_gain, y_xoffset                      with d_in = k(k+3)/2.
 * Any tansig MLP with one hidden width <= 64 and <= 4 hidden layers is accepted.  The input domain of a network is
 * x_i in [0, 1] (the first k inputs) and q_m in [-1/k, 1/k] (Q_slice / max_elem); input i is mapped by
 * v -> (v - xoffset_i) gain_i + ymin.  On that domain every score kernel computes the network itself.  A network whose hidden
 * pre-activations are provably below 40 for mapped inputs in [-3, 3] AND whose mapping sends the domain into [-3, 3] runs the
 * clamp-free variant of the MFMA kernel, which cuts a mapped input outside [-3, 3] -- an LP point beyond the box -- at +-3;
 * every other network runs the variant that clamps the tansig arguments and no input.
 * Replacing the network of a size class invalidates the optimality scores of the current list (they are computed again by the
 * next call that needs them).
 */
int sdpcut_set_network(sdpcut_handle h, int k, int n_layers, const int32_t *widths,
                       const double *params, int64_t n_params);

/* The four trained MLPs of the reference (k = 2 .. max_k), compiled into the library from
 * data/nn_weights.npz: sdpcut_set_network for each of them without the caller holding weights. */
int sdpcut_set_builtin_networks(sdpcut_handle h, int max_k);

/* Instance table: packed row-major upper triangle of the objective, length n(n+1)/2
 * (self._Q_arr, cut_select_qp.py:318-321 / cut_select_qcqp.py:247-256). */
int sdpcut_set_instance(sdpcut_handle h, int32_t nb_vars, const double *Q_arr);

/*
 * Candidate index sets (self._agg_list[i][0], cut_select_qp.py:529-540).  set_inds is
 * [N][ld] int32 with the first ks[i] entries of row i valid (2 <= ks[i] <= 5, ld >= max k);
 * Xarr_inds, Q_slice and max_elem are re-derived on the device from Q_arr.
 * global_base is added to every candidate index this handle reports (multi-GPU shards).
 */
int sdpcut_set_candidates(sdpcut_handle h, int64_t N, const int32_t *set_inds, int32_t ld,
                          const int32_t *ks, int64_t global_base);

/*
 * The C4 workload of SURVEY.md section 8 d, generated in device memory: N random k-variable index
 * sets, candidate id -> set through a counter-based generator (Philox4x32-10 keyed by `seed`,
 * counter = (id, attempt, block); k draws floor(u32 * nb_vars / 2^32), sorted, redrawn until
 * distinct: every k-subset equally likely, ids independent of each other and of N).  The handle's
 * list becomes the ids first_id .. first_id + N - 1, which are also the GLOBAL indices it reports
 * (shard r of a multi-GPU run passes first_id = r * N).  Replaces, for synthetic batches, the
 * host-built list of sdpcut_set_candidates; csrc/philox.h is the arithmetic, synthetic.py its
 * numpy twin.  Needs nb_vars >= 2 k.
 */
int sdpcut_set_candidates_philox(sdpcut_handle h, int32_t k, int64_t N, uint64_t seed, int64_t first_id);

/*
 * Semidefinite vertex cover P^E_dim enumerated on the device, straight into the handle's candidate
 * list (replaces _get_sdp_vertex_cover's index-set loops, cut_select_qp.py:399-524, AND the upload
 * of their result): same sets, same order as sdpcut_enumerate_cover.  adjacency as there
 * ([nb_vars][nb_vars] bytes, nb_vars of sdpcut_set_instance, <= 1024).  *count_out = number of
 * candidates.  max_subs > 0 mirrors the reference's RAM guard (_THRES_MAX_SUBS, :117-120): with
 * count >= max_subs only the count is returned and the handle's list is left alone; 0 = no guard.
 */
int sdpcut_set_candidates_cover(sdpcut_handle h, const uint8_t *adjacency, int32_t dim, int64_t max_subs,
                                int64_t *count_out);

/*
 * The covers on a chordal extension of the sparsity pattern (ch_ext of _get_sdp_vertex_cover, cut_select_qp.py:385-455), on the
 * device: same sets, same order as the host twins.  adjacency_orig is the pattern of Q, adjacency_ext its chordal extension
 * (sdpcut_chordal_extension, or the caller's own); both as in sdpcut_set_candidates_cover.
 *   ch_ext =  0  P^E_dim: sdpcut_set_candidates_cover on adjacency_orig (adjacency_ext may be NULL);
 *   ch_ext =  1  P^bar(E)_dim: the same enumeration on adjacency_ext (adjacency_orig may be NULL), any dim 3..5 -- what the
 *                reference's loops do once Q_adj is replaced (:396);
 *   ch_ext =  2  bar(P*_3), :429-449: triangles of the extended graph with at least 2 of their 3 edges in the original one, and
 *                the original edges that belong to none (sdpcut_enumerate_cover_ch).  dim must be 3: the reference silently
 *                degrades ch_ext = 2 to ch_ext = 1 at dim 4 and 5 (:456-522 never look at it), this call refuses it;
 *   ch_ext = -1  P^E+_3, :450-455: all triples = the dim-3 cover of the complete graph (both adjacencies may be NULL); dim 3 only.
 * Guards, count_out and max_subs as in sdpcut_set_candidates_cover.
 */
int sdpcut_set_candidates_cover_ch(sdpcut_handle h, const uint8_t *adjacency_ext, const uint8_t *adjacency_orig, int32_t ch_ext,
                                   int32_t dim, int64_t max_subs, int64_t *count_out);

/*
 * The two candidate lists of a QCQP instance (replaces __get_vertex_cover, cut_select_qcqp.py:314-334, including its
 * list-membership intersection): h_in receives the sub-problems of the cover of `adjacency_all` (objective + all
 * constraints) that also belong to the cover of `adjacency_obj` (self._agg_list, :331), h_out the others
 * (agg_list_cons, :332-333), both in the order of the `adjacency_all` enumeration.  Everything happens on the device
 * (two enumerations, one binary search per set, prefix sums); the handles must sit on the same device and hold the
 * same instance (sdpcut_set_instance).  Adjacencies as in sdpcut_set_candidates_cover.
 */
int sdpcut_set_candidates_cover_split(sdpcut_handle h_in, sdpcut_handle h_out, const uint8_t *adjacency_obj,
                                      const uint8_t *adjacency_all, int32_t dim, int64_t *n_in, int64_t *n_out);

/* Index sets of `count` candidates given by LOCAL index, device -> host: set_inds_out [count][5]
 * padded with -1, ks_out [count] (0 for an index outside the list).  For lists that were generated
 * or enumerated on the device: the host names only the few thousand selected candidates. */
int sdpcut_get_candidates(sdpcut_handle h, int64_t count, const int64_t *idx, int32_t *set_inds_out,
                          int32_t *ks_out);

/* LP point vars_values = [X packed (L) | x (n)]  (cut_select_qp.py:137, 200, 547). */
int sdpcut_set_point(sdpcut_handle h, const double *vars_values);
/* The handle's pinned, device-mapped staging block for the LP point: *buf = (L + n) doubles the caller may fill IN PLACE
 * (let the LP solver write its solution there) and then pass to sdpcut_set_point / sdpcut_round_view / sdpcut_round_csr,
 * which recognise the pointer and skip their host copy (4 MB at n = 1000: ~110 us per round).  Valid until the next
 * sdpcut_set_instance; write to it only between rounds (a round's completion means its point has left the host). */
int sdpcut_point_buffer(sdpcut_handle h, double **buf);
/* same, from a device buffer (async copy on the handle's stream) */
int sdpcut_set_point_device(sdpcut_handle h, const void *d_vars_values);

/*
 * Node box: the variable bounds l <= x <= u of a node of a spatial branch and bound (the reference assumes [0, 1] throughout,
 * cut_select_qcqp.py:275-276).  The small SDP the MLP estimates carries the secant of the unit box, X_ii <= x_i; at a node the valid
 * constraint is X_ii <= (l_i + u_i) x_i - l_i u_i.  The problem is affine-invariant: with d = u - l and x = l + D x' the node problem in
 * x' IS the unit-box problem the networks were trained on, on the tables
 *     x'_i  = (x_i - l_i) / d_i
 *     X'_ij = (((X_ij - l_i x_j) - l_j x_i) + l_i l_j) / (d_i d_j)      i <= j, diagonal included
 *     Q'_ij = Q_ij (d_i d_j)
 * (fp64, this operation order, no contraction: on the unit box all three equal the originals bit for bit), and the affine terms in
 * x cancel between <Q, X> and the minimum, so the measure stays the objective improvement in the ORIGINAL units -- comparable
 * across nodes and with BIG_M.  csrc/box.hip writes Q' once per sdpcut_set_box and the transformed point once per LP point, in
 * stream order behind the point's copy (one launch more per round).
 * With a box set SDPCUT_NN and SDPCUT_SDP are computed from the transformed tables; lambda_min (SDPCUT_EIG), the violated test,
 * the eigenvectors and every cut row from the original point as before (PSD cuts do not depend on bounds): strategies 0, 1 and 5
 * are unaffected.  A call that scores SDPCUT_EIG | SDPCUT_NN runs two launches, and a round scores first and then takes the
 * selection of an already scored list (no fused launch, no SDPCUT_OPT_SKIP_NONVIOLATED).  With SDPCUT_OPT_TIMING the score time
 * of such a two-launch call is the LAST launch's (the MLP's): both dispatches carry the same pair of events.  What a boxed round
 * costs next to the plain round of the same list, and what it gains in bound per round: tools/node_rounds.py ->
 * profiles/node_rounds.txt, run on two short lists only (single samples: 5-12 % more per round at 243 candidates; at 6608
 * candidates level under strategy 2 and up to ~40 % more under strategy 4; no bound gain beyond the scatter between nodes);
 * long lists are not measured.  DESIGN.md section 5 "Node boxes".
 * lb, ub: [nb_vars] each, 0 <= lb_i < ub_i <= 1 and ub_i - lb_i >= SDPCUT_BOX_MIN_WIDTH (ten halvings of a variable; the division
 * amplifies rounding by ~ 8 eps / (d_i d_j) absolute on X'), else SDPCUT_EINVAL: fixed and nearly fixed variables are a limitation.
 * Both NULL clears the box.  Clears the SDPCUT_NN and SDPCUT_SDP bits of the scores at the current point and keeps SDPCUT_EIG; a
 * current point is transformed again.  sdpcut_set_instance clears the box.
 * Refused while a box is set (SDPCUT_ESTATE, handle unchanged): sdpcut_score_points and sdpcut_round_csr_points (one Q for all
 * points) and their boxed forms sdpcut_score_points_boxed / sdpcut_round_csr_points_boxed (a box per point, passed with the
 * call: the handle's own would be lost), the sharded entry points (sdpcut_shard_*), and switching SDPCUT_OPT_EXACT_HEAD on (reference-exact
 * bits have no meaning where the reference has no boxes); sdpcut_set_box refuses a box while that option is on.
 */
#define SDPCUT_BOX_MIN_WIDTH 0.0009765625 /* 2^-10 */
int sdpcut_set_box(sdpcut_handle h, const double *lb, const double *ub);
/* the box ([nb_vars] each, either may be NULL; [0, 1] when none is set) and whether one is set */
int sdpcut_get_box(sdpcut_handle h, double *lb, double *ub, int *is_set);
/* The transformed tables as the kernels read them: Q_box [L], vars_box [L + n] (either may be NULL).  SDPCUT_ESTATE without a box;
 * vars_box needs a current point.  Waits for the handle's stream. */
int sdpcut_get_box_tables(sdpcut_handle h, double *Q_box, double *vars_box);

/*
 * Score every candidate at the current point (replaces the per-candidate loop bodies of
 * _sel_eigcut_by_ordering_on_measure, cut_select_qp.py:570-582 and :642-648):
 *   SDPCUT_EIG: eigmin[i]      = lambda_min([[1, x^T],[x, X]])          (a6; numpy.linalg.eigvalsh(...)[0] at cut_select_qp.py:796.
 *               (r4) Householder tridiagonalisation + Laguerre's iteration, Jacobi for nearly multiple lambda_min (csrc/lmin.h):
 *               as far from the exact eigenvalue as LAPACK is, ~1e-16 on average, <= 2e-15 against LAPACK on matrices of norm 2-4)
 *   SDPCUT_NN : obj_improve[i] = (-S) * max_elem + nn([x | Q_slice]) * max_elem  (a4, a5)
 *   SDPCUT_SDP: obj_exact[i]   = (-S) * max_elem + p*_lower * max_elem   (cut_select_qp.py:575, :595 -- the MOSEK call of strategy 3,
 *               :586-598).  p* = min sum_{i<=j} q_ij X_ij  s.t. [[X, x],[x^T, 1]] >= 0, X_ii <= x_i  with x = x_rho and q = Q_slice, the
 *               MLP's own input.  With Y = X - x x^T, C_ii = q_ii, C_ij = q_ij / 2, d_i = max(x_i - x_i^2, 0):
 *                   p* = sum q_ij x_i x_j + min{ <C, Y> : Y >= 0, Y_ii <= d_i } = sum q_ij x_i x_j - min{ d^T lam : lam >= 0, C + Diag(lam) >= 0 }
 *               solved per candidate, one lane each, by a dual barrier method (csrc/exact_sdp.h) that keeps a CERTIFICATE: a dual
 *               feasible lam (lower bound p*_lower, what the score uses) and a primal feasible Y (upper bound); gap[i] = upper - lower
 *               >= 0 in the normalised units of p*.  Stops at gap <= 1e-9 max(1, |p*|) or at an iteration cap
 *               (SDPCUT_STAT_SDP_UNCONVERGED counts the latter).  Rules: an index with d_i = 0 (x_i on or outside its bounds) is
 *               eliminated -- row and column i of Y are zero, lam_i is reported as 0; if the scaled C is positive semidefinite already
 *               the answer is lam = 0, Y = 0, p* = sum q_ij x_i x_j.  Needs an instance, candidates and a point -- NO networks; its own
 *               arrays: eigmin / obj_improve and their scored bits are untouched.  Fetch with sdpcut_get_sdp_scores.
 * Results stay on the device; fetch with sdpcut_get_scores.
 */
int sdpcut_score(sdpcut_handle h, uint32_t flags);
int sdpcut_get_scores(sdpcut_handle h, double *eigmin, double *obj_improve); /* either may be NULL */

/*
 * SDPCUT_EFF: efficacy of the eigen-cut a round would emit for candidate i at the current point (csrc/efficacy.hip; efficacy.py is
 * the numpy twin).  lam = eigmin[i], the lambda_min the handle holds -- scoring SDPCUT_EFF scores SDPCUT_EIG first if it is missing
 * -- and coef[0 .. M), cols[0 .. M), M = k + k(k+1)/2, exactly what sdpcut_cut_rows returns for i (the same device function with the
 * same lam: the row a round emits, not another vector of the eigenspace).  In fp64, sums in column order m = 0 .. M-1, no
 * contraction, IEEE square root and division:
 *     nrm       = sqrt(sum coef[m]^2)
 *     violated  : lam < -1e-15 and nrm > 0
 *     eff[i]    = -lam / nrm                 (violated)       the Euclidean distance by which the row cuts off the LP point
 *               = min(-lam, +0.0)            (otherwise; such a candidate costs no eigenvector)      => eff > 0 <=> violated
 *     objpar[i] = |sum coef[m] obj[cols[m]]| / (nrm ||obj||_2)   (violated, an objective vector set), else 0.0
 *     escore[i] = eff[i] + w objpar[i]       (violated), else eff[i]
 * Like lambda_min and the rows the measure is computed from the ORIGINAL point: a node box (sdpcut_set_box) does not change it, and
 * sdpcut_set_box leaves its scored bit alone.  No networks needed.  Whatever clears SDPCUT_EIG clears SDPCUT_EFF.
 *
 * sdpcut_set_objective: the LP objective in the column layout of vars_values, n_cols = n(n+1)/2 + n entries; obj == NULL clears it.
 *   ||obj||_2 is computed once here, on the host: squares summed in index order without contraction, IEEE square root.
 *   SDPCUT_EINVAL (the handle unchanged): a length mismatch, a non-finite entry, an all-zero vector.  Needs sdpcut_set_instance, which
 *   also clears the vector.
 * sdpcut_set_efficacy_weight: w, finite and >= 0 (SDPCUT_EINVAL otherwise); the default 0 ranks by pure efficacy, SCIP's default
 *   weights correspond to w = 0.1.
 * Both clear SDPCUT_EFF only and are refused with SDPCUT_ESTATE while a round is pending.
 * sdpcut_get_efficacy: eff, objpar, escore [N] each in caller order, any may be NULL; SDPCUT_ESTATE unless SDPCUT_EFF is scored at
 *   the current point.
 */
int sdpcut_set_objective(sdpcut_handle h, int64_t n_cols, const double *obj);
int sdpcut_set_efficacy_weight(sdpcut_handle h, double w);
int sdpcut_get_efficacy(sdpcut_handle h, double *eff, double *objpar, double *escore);
/* the exact measure and its duality gap (either may be NULL); SDPCUT_ESTATE unless SDPCUT_SDP has been scored at the current point */
int sdpcut_get_sdp_scores(sdpcut_handle h, double *obj_exact, double *gap);

/*
 * Rank (replaces the sorts / combined scan, cut_select_qp.py:601-632 and :649-654).
 *   strat 1: violated candidates (lambda_min < -1e-15) by -lambda_min descending
 *   strat 2: all candidates by obj_improve descending
 *   strat 3: all candidates by the exact measure of SDPCUT_SDP descending (only with SDPCUT_OPT_EXACT_SDP, see there)
 *   strat 4: combined scan with BIG_M, using sel_size; *new_strat = 1 or 4 (:630-631)
 *   strat 6: all candidates by the efficacy score of SDPCUT_EFF descending (SDPCUT_STRAT_EFF, see there)
 * Ties keep ascending candidate index (Python's stable sort).  Writes the first
 * min(max_out, length) entries: idx_out = global candidate index, score_out = ranking score.
 * *n_total = full length of the reference's list (N, or nb_violated for strat 1).
 * counters (may be NULL) = {nb_violated, strong_violated, violated_in_scan, nb_positive}.
 * Requires a preceding sdpcut_score with the flags the strategy needs.
 */
int sdpcut_rank(sdpcut_handle h, int strat, int64_t sel_size, int64_t max_out,
                int64_t *idx_out, double *score_out, int64_t *n_total,
                int32_t *new_strat, int64_t *counters);
/* same, writing to device buffers (for the multi-GPU all-gather); returns counts on host */
int sdpcut_rank_device(sdpcut_handle h, int strat, int64_t sel_size, int64_t max_out,
                       void *d_idx_out, void *d_score_out, int64_t *n_written,
                       int64_t *n_total, int32_t *new_strat, int64_t *counters);

/* Read entries [offset, offset+count) of the ranking produced by the last sdpcut_rank /
 * sdpcut_rank_device call (the reference hands back the whole sorted list; callers normally
 * consume only its head, so the tail stays on the device until asked for).  A ranking whose head came from the top-k selection
 * (max_out <= 16384 and no void selection) has no tail on the device: the call then fails with SDPCUT_ESTATE, as it does before
 * the first ranking and after sdpcut_set_point, sdpcut_set_candidates, sdpcut_set_box, sdpcut_tri_separate and a batched call.
 * Which of the two a ranking is depends on the list, the scores, the options and the arguments alone, not on earlier calls. */
int sdpcut_rank_fetch(sdpcut_handle h, int64_t offset, int64_t count, int64_t *idx_out,
                      double *score_out);

/*
 * Order `count` entries by (score descending, secondary descending, id ascending) and write
 * the first max_out: the replicated merge after the all-gather of per-shard top-k (SURVEY
 * 8 e).  d_secondary may be NULL (two-level key).  The secondary key carries obj_improve for
 * the combined strategy, whose second stable sort keeps first-sort order among equal new
 * scores (cut_select_qp.py:601, :625).  All pointers are device pointers; ids are int64.
 */
int sdpcut_merge_topk_device(sdpcut_handle h, int64_t count, const void *d_scores,
                             const void *d_secondary, const void *d_ids, int64_t max_out,
                             void *d_score_out, void *d_id_out);

/* eigmin / obj_improve of `count` candidates given by GLOBAL index, device to device
 * (either output may be NULL). */
int sdpcut_gather_scores_device(sdpcut_handle h, int64_t count, const void *d_ids,
                                void *d_eig_out, void *d_obj_out);

/*
 * Eigen-cut rows of selected candidates (replaces the loop body of _gen_eigcuts_selected,
 * cut_select_qp.py:737-750).  idx are LOCAL candidate indices (global - global_base).
 *   lam_min[c]                 smallest eigenvalue
 *   coef[c*SDPCUT_ROW_LD + .]  [2v0v1..2v0vk | v1^2, 2v1v2, .., vk^2] with |v_i|<=1e-15 zeroed
 *   rhs[c]                     -v0^2
 *   cols[c*SDPCUT_ROW_LD + .]  [L + i for i in set_inds] + Xarr_inds   (int64)
 *   ks[c]                      candidate size k (row length = k + k(k+1)/2)
 * A row is only meaningful when lam_min < -1e-15 (the reference skips the others).
 * v = unit eigenvector of lam_min (numpy.linalg.eigh at cut_select_qp.py:796-797): inverse iteration with lam_min (LU of
 * A - lam I, residual a few ulp of ||A||) -- the value the handle holds for the candidate at the current point (SDPCUT_EIG scored,
 * e.g. by a feasibility / combined round) or, (r4) when it holds none, the value the same solver computes on the spot
 * (Householder + Laguerre, csrc/lmin.h).  Whenever lam_min is multiple or within 1e-10 ||A|| of the next eigenvalue, where only an
 * eigenSPACE is defined, v comes from a Jacobi iteration with vectors.  Either way the row is a unit
 * eigenvector's cut; two solvers agree on it to eps / gap, as the reference's LAPACK and this library always did.
 */
int sdpcut_cut_rows(sdpcut_handle h, int64_t count, const int64_t *idx, double *lam_min,
                    double *coef, double *rhs, int64_t *cols, int32_t *ks);

/*
 * One selection round in one call: what the loop body does between two LP solves
 * (cut_select_qp.py:165-182: _sel_eigcut_by_ordering_on_measure followed by
 * _gen_eigcuts_selected).  Scores with the flags the strategy needs (unless already scored
 * at this point), ranks, and produces the eigen-cut rows of the first min(sel_size, length)
 * entries; a single device-to-host transfer returns everything.  Outputs are sized for
 * sel_size entries; *n_out entries are written.  idx_out are GLOBAL candidate indices;
 * the column indices of row c follow from its index set (see sdpcut_cut_rows) and are not
 * transferred.  lam_min / coef / rhs / ks as in sdpcut_cut_rows, except that coef rows have
 * the caller's stride coef_ld (>= k + k(k+1)/2 of the largest candidate, <= SDPCUT_ROW_LD):
 * a 3-variable-only list moves 9 instead of 20 doubles per row over PCIe.
 */
int sdpcut_select_round(sdpcut_handle h, int strat, int64_t sel_size, int32_t coef_ld,
                        int64_t *idx_out, double *score_out, double *lam_min, double *coef,
                        double *rhs, int32_t *ks, int64_t *n_out, int64_t *n_total,
                        int32_t *new_strat, int64_t *counters);
/*
 * Zero-copy form: the device writes the round's results straight into a pinned host block owned
 * by the handle; *block points at it and stays valid until the next call on the handle.  With
 * cap = *cap_out = min(sel_size, N) the block is
 *     64 bytes reserved | int64 idx[cap] | double score[cap] | double lam_min[cap] |
 *     double rhs[cap] | double coef[cap][coef_ld] | int32 ks[cap]
 * of which the first *n_out entries of every array are meaningful (*block is NULL if cap = 0).
 */
int sdpcut_select_round_view(sdpcut_handle h, int strat, int64_t sel_size, int32_t coef_ld,
                             const void **block, int64_t *cap_out, int64_t *n_out,
                             int64_t *n_total, int32_t *new_strat, int64_t *counters);

/*
 * One cutting-plane round from the LP point to the cut rows in ONE call: sdpcut_set_point(vars_values)
 * followed by sdpcut_select_round_view(...) -- what the separation step of cut_select_qp.py:165-182
 * does between two LP solves.  Same results as the two calls; the point transfer and the score kernel are
 * enqueued back to back and the caller crosses the FFI once per round.
 */
int sdpcut_round_view(sdpcut_handle h, const double *vars_values, int strat, int64_t sel_size, int32_t coef_ld,
                      const void **block, int64_t *cap_out, int64_t *n_out,
                      int64_t *n_total, int32_t *new_strat, int64_t *counters);

/*
 * One cutting-plane round with the cuts ASSEMBLED: everything the separation step of cut_select_qp.py:165-182 hands
 * to the LP -- _sel_eigcut_by_ordering_on_measure (:543-703), _gen_eigcuts_selected (:705-755) and the row objects
 * the latter builds one cut at a time (cplex.SparsePair(ind=[L + i for i in set_inds] + Xarr_inds, val=coeffs),
 * rhs -v0^2, sense "G"; :744-750) -- as one block of rows in compressed sparse row form, assembled on the device
 * and stored straight into a pinned host block owned by the handle (SURVEY.md section 8 f row 4).
 *
 * vars_values: the LP point [X packed | x] (sdpcut_set_point is part of the call), or NULL to keep the current one.
 * sel_size: the strategy's quota AND the number of head entries returned (cap = min(sel_size, N)).
 * All pointers of *out point INTO the handle's block: valid until the next call on the handle, never freed by the caller.
 *   head (n_out entries, rank order):  idx (global candidate ids), score, lam_min (NaN for a candidate of another
 *       shard), ks (candidate size), set_inds [.][5] (index sets padded with -1)
 *   cuts (n_rows <= n_out; an entry yields one iff its lam_min < -1e-15, :739), in head order:
 *       row_entry[r] = head position of cut r;  rhs[r];  indptr[r] .. indptr[r + 1] = its span in indices / values
 *       (n_rows + 1 entries, indptr[n_rows] = nnz);  indices = LP columns (:747),  values = coefficients (:745-746).
 * The cuts of the first m head entries are rows 0 .. r-1 with r = #{row_entry < m} (row_entry ascends), i.e. a
 * prefix of the block: a caller that consumes fewer entries (strong_only, :725-726) slices, nothing is recomputed.
 */
typedef struct sdpcut_round_csr {
    int64_t cap, n_out, n_total;
    int32_t new_strat;
    int32_t row_ld;                 /* longest possible row (k + k(k+1)/2 of the largest candidate size): indices / values hold cap * row_ld */
    int64_t counters[4];            /* as sdpcut_rank */
    const int64_t *idx;
    const double *score;
    const double *lam_min;
    const int32_t *ks;
    const int32_t *set_inds;
    int64_t n_rows, nnz;
    const int32_t *row_entry;
    const int32_t *indptr;
    const int32_t *indices;
    const double *values;
    const double *rhs;
} sdpcut_round_csr_t;
int sdpcut_round_csr(sdpcut_handle h, const double *vars_values, int strat, int64_t sel_size, sdpcut_round_csr_t *out);
/* The same in two halves: _begin enqueues the whole round and returns without waiting, _end waits and fills *out (and runs the
 * general ranking path itself in the rare cases the enqueued selection is not the answer).  A handle holds one pending round;
 * DIFFERENT handles may all begin before any ends -- their device work overlaps.  The QCQP round ranks two lists per LP point
 * (cut_select_qcqp.py:64-78): begin(objective cover), begin(constraints cover), end, end. */
int sdpcut_round_csr_begin(sdpcut_handle h, const double *vars_values, int strat, int64_t sel_size);
int sdpcut_round_csr_end(sdpcut_handle h, sdpcut_round_csr_t *out);

/*
 * Many LP points against ONE candidate list per call: the open nodes of a branch-and-bound tree, the children of a dive, the
 * candidate points of a strong-branching step.  A single round on a short list costs its launch chain and the host hand-off, not
 * arithmetic; these calls pay both once for n_points points.
 *
 * points: n_points rows of L + n doubles ([X packed | x], as sdpcut_set_point takes them), row p at points + p * point_ld,
 * point_ld >= L + n.  1 <= n_points <= SDPCUT_BATCH_MAX_POINTS (SDPCUT_EINVAL beyond).  Both calls are synchronous, need an
 * instance and candidates (SDPCUT_ESTATE without), refuse a handle with a pending round (sdpcut_round_csr_begin,
 * sdpcut_shard_finish_enqueue: SDPCUT_ESTATE) and LEAVE THE HANDLE WITHOUT A CURRENT POINT: nothing is scored afterwards, and a
 * single-point call that follows needs its own sdpcut_set_point (sdpcut_score, sdpcut_rank ... fail with SDPCUT_ESTATE until
 * then; sdpcut_round_csr with a point is fine).  The handle's single-point arrays are scratch of the per-point fallback.
 *
 * sdpcut_score_points: flags = any combination of SDPCUT_EIG | SDPCUT_NN (SDPCUT_SDP and SDPCUT_EFF are refused in this version).  eig_out /
 * obj_out: host arrays [n_points][N], row p = what sdpcut_set_point(point p), sdpcut_score(flags), sdpcut_get_scores returns, bit
 * for bit; the array of a measure that is not asked for may be NULL (one that is asked for may not).  One point copy and one
 * score launch with a point axis per size class (an eigenvalue-only scan: one launch).
 *
 * sdpcut_round_csr_points: out[p] is what sdpcut_round_csr(h, points + p * point_ld, strat, sel_size, &o) returns -- every field
 * and every array, bit for bit.  Strategies 1, 2 and 4 are served; 0, 3, -1, 5, 6 and the SDPCUT_PART_* codes are refused with
 * SDPCUT_EINVAL.  All pointers of out[0 .. n_points) point into ONE pinned block of the handle (point p's slice starts with its
 * own header and is 64-byte aligned); they stay valid until the next call on the handle.
 *   Lists of at most 4096 candidates with a head of 1 .. 512 entries (SDPCUT_OPT_EXACT_HEAD off, no shard base): one point copy,
 *   one score launch per size class, ONE selection launch (a workgroup per point selects, sorts and emits its head), ONE row
 *   assembly, ONE host wait.  A point whose selection declared itself void is served by the single-point round inside the call
 *   (SDPCUT_STAT_POINTS_REDONE counts them).
 *   Everything else -- longer lists, longer or empty heads, exact heads, a kernel variant without a point axis -- runs the
 *   single-point round once per point inside the call and copies each result into the point's slice.
 */
#define SDPCUT_BATCH_MAX_POINTS 256
int sdpcut_score_points(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, uint32_t flags, double *eig_out,
                        double *obj_out);
int sdpcut_round_csr_points(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, int strat, int64_t sel_size,
                            sdpcut_round_csr_t *out /* [n_points] */);

/*
 * The same two calls with a NODE BOX PER POINT (sdpcut_set_box): the open nodes of a tree search, each with its own LP point and
 * its own variable bounds.  Row p of lb / ub (row p at lb + p * box_ld, box_ld >= n) is the box of point p; a [P][2][n] array is
 * passed as lb = boxes, ub = boxes + n, box_ld = 2 n.
 *   Row p of the result is, bit for bit, what sdpcut_set_box(h, lb_p, ub_p) followed by the single-point call at point p returns
 *   on a fresh handle: scores, heads, every CSR array, n_total, new_strat and the counters.
 *   Every box is checked with sdpcut_set_box's rule before any state changes (SDPCUT_EINVAL; the message names the point and the
 *   variable).  A handle that has a box of its own is refused (SDPCUT_ESTATE) and keeps it, like the unboxed calls;
 *   SDPCUT_OPT_EXACT_HEAD on is refused as sdpcut_set_box refuses it (SDPCUT_ESTATE), a pending round as everywhere.  Flags,
 *   strategies and n_points are those of the unboxed calls.  After either call the handle has NO CURRENT POINT AND NO BOX,
 *   whichever way the call returns.
 *   One-wait route: under the conditions of sdpcut_round_csr_points, and while the per-point tables -- n_points (2 L + n) doubles:
 *   Q' and the transformed point of every point -- fit 256 MiB.  The (l | d) rows travel with the points; one launch with a point
 *   axis writes every Q'_p and transformed point (csrc/box.hip: box_points_kernel); lambda_min is scored on the original points,
 *   the measure by the MFMA launch on the transformed ones with a Q stride of L; the combined strategy's strong class is counted
 *   per point by a small kernel (neither launch sees both measures); selection and row assembly are the unboxed batch's.  A scan
 *   that asks for SDPCUT_EIG alone, and a strategy-1 batch, need no box table at all.  A point whose selection declared itself
 *   void goes through sdpcut_set_box and the single-point round inside the call.
 *   Everything else loops inside the call: sdpcut_set_box and the single-point round per point, the box cleared at the end.
 */
int sdpcut_score_points_boxed(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, const double *lb, const double *ub,
                              int64_t box_ld, uint32_t flags, double *eig_out, double *obj_out);
int sdpcut_round_csr_points_boxed(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, const double *lb, const double *ub,
                                  int64_t box_ld, int strat, int64_t sel_size, sdpcut_round_csr_t *out /* [n_points] */);

/*
 * Diverse selection: a parallelism filter on the ranked head.  A round takes the first sel_size entries of its ranking however
 * similar their cuts are; candidates that share two of three variables share five of nine LP columns and their eigen-cuts are often
 * nearly the same row.  These calls walk a POOL in rank order and accept an entry only if its cut is not too parallel to the cuts
 * accepted before it -- the second criterion of every MIP solver's cut selector.  The rule ("Diverse selection"):
 *   row a_t of entry t    what sdpcut_cut_rows gives for the candidate at the current point, on its LP columns
 *                         [L + i for i in set_inds] + Xarr_inds; the right-hand side takes no part
 *   eligible              lam_min < -1e-15 and ||a_t|| > 0
 *   walk t = 0, 1, ...    an eligible entry is accepted iff fewer than the quota are accepted so far and every accepted s has
 *                         |<a_s, a_t>| <= max_parallel ||a_s|| ||a_t||  (inner product over the shared LP columns: x_c for every
 *                         common variable c, X_cd for common c <= d; compared without a division)
 *   max_parallel >= 1     no comparison at all: the first `quota` eligible entries (a list may hold a candidate twice)
 * The walk ends with the entry that fills the quota.  info: pool = entries of the pool, examined = entries the walk looked at,
 * skipped_nonviolated = those that were not eligible, rejected_parallel = eligible ones refused as parallel
 * (examined = accepted + skipped_nonviolated + rejected_parallel).
 *
 * sdpcut_round_csr_diverse: one round as sdpcut_round_csr (vars_values NULL keeps the current point), strategies 1, 2, 4 and 6.  The
 * pool is the first min(pool_size, length) entries of what sdpcut_rank(h, strat, sel_size, max_out = pool_size, ...) returns --
 * sel_size stays the combined strategy's quota; n_total, new_strat and counters are those of that call; SDPCUT_OPT_EXACT_HEAD is
 * honoured as that call honours it.  *out is the block of sdpcut_round_csr for the ACCEPTED entries in rank order: cap =
 * min(sel_size, pool), n_out accepted entries, every one with its row (n_rows == n_out, row_entry[r] == r).  Synchronous; the
 * pointers stay valid until the next call on the handle.  With max_parallel = 1 and pool_size = sel_size the block equals that of
 * sdpcut_round_csr restricted to its cut-yielding entries, bit for bit.
 *
 * sdpcut_filter_parallel: the same walk over `count` candidates in an order the CALLER supplies (local ids; a QCQP caller's
 * concatenated list, a merged sharded head, a ranking of one's own) at the current point: keep_out[i] = 1 iff entry i is accepted.
 *
 * SDPCUT_EINVAL: a strategy outside {1, 2, 4, 6}, max_parallel outside [0, 1] or NaN, sel_size / quota < 1, pool_size < sel_size, a
 * pool or count above SDPCUT_DIVERSE_MAX_POOL, an id outside the list.  SDPCUT_ESTATE: no instance, candidates or point; a round
 * pending.  Device memory: per pool entry 250 bytes, and -- only when max_parallel < 1 -- the lower-triangular bit matrix of the pair
 * test, 16.8 MB at a pool of 16384 (4 KB at 256); allocated by the first call, grown to the largest pool, freed with the handle.
 */
#define SDPCUT_DIVERSE_MAX_POOL 16384
typedef struct sdpcut_diverse_info { int64_t pool, examined, skipped_nonviolated, rejected_parallel; } sdpcut_diverse_info_t;
int sdpcut_round_csr_diverse(sdpcut_handle h, const double *vars_values, int strat, int64_t sel_size, int64_t pool_size,
                             double max_parallel, sdpcut_round_csr_t *out, sdpcut_diverse_info_t *info);
int sdpcut_filter_parallel(sdpcut_handle h, int64_t count, const int64_t *idx, int64_t quota, double max_parallel, uint8_t *keep_out,
                           sdpcut_diverse_info_t *info);

/*
 * Efficacy and the filtered round over MANY LP POINTS (points, point_ld, n_points, the refusals and the state afterwards as for
 * sdpcut_score_points / sdpcut_round_csr_points: no current point, nothing scored -- SDPCUT_EFF included -- and no box).
 *
 * sdpcut_efficacy_points: row p of eff_out / objpar_out / escore_out ([n_points][N] each; any may be NULL, not all) is what
 * sdpcut_set_point(point p), sdpcut_score(SDPCUT_EIG | SDPCUT_EFF), sdpcut_get_efficacy returns, bit for bit, with the handle's
 * objective and weight.  One point copy, the eigenvalue launch and one efficacy launch with a point axis.  Efficacy knows no box.
 *
 * sdpcut_round_csr_points_diverse: out[p] and info[p] (info may be NULL) are what sdpcut_round_csr_diverse(h, point p, strat,
 * sel_size, pool_size, max_parallel, &o, &i) returns -- every field, every array, n_total, new_strat and the counters, bit for bit;
 * strategies 1, 2, 4 and 6.  lb / ub (both NULL: no boxes; else rows of box_ld >= n doubles as for sdpcut_round_csr_points_boxed):
 * the comparison call then follows sdpcut_set_box(h, lb_p, ub_p) on a fresh handle; the boxes are checked before any state changes,
 * a handle with a box of its own or SDPCUT_OPT_EXACT_HEAD on is refused.  Strategies 1 and 6 read no box.  All pointers point into
 * one pinned block of the handle (slices of the layout for cap = min(sel_size, pool)), valid until the next call on the handle.
 * SDPCUT_EINVAL: the cases of sdpcut_round_csr_diverse and those of sdpcut_round_csr_points for n_points and point_ld.
 *   One-wait route (SDPCUT_STAT_DIVERSE_POINTS_FAST counts its points): lists of at most 4096 candidates, pool = min(pool_size, N)
 *   of 1 .. 512 entries, SDPCUT_OPT_EXACT_HEAD off, no shard base, boxed: the box tables within 256 MiB; strategy 4 only with
 *   min(sel_size, N) == pool (its ranking depends on the quota; csrc/batch_route.h: batch_route_diverse).  One point copy, the score
 *   launches of the batched round (strategy 6: eigenvalues, then the efficacy launch), one selection launch with k = pool, one row
 *   launch for the pools, ONE filter launch -- a workgroup per point holds the pool's rows, index sets and pair bits in LDS and walks
 *   it (csrc/diverse.hip: div_points_kernel) -- one row assembly over the accepted heads, ONE host wait.  A point whose selection
 *   declared itself void goes through the single-point call (SDPCUT_STAT_POINTS_REDONE).
 *   Everything else loops inside the call: sdpcut_set_box where there are boxes, then sdpcut_round_csr_diverse per point.
 */
int sdpcut_efficacy_points(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, double *eff_out, double *objpar_out,
                           double *escore_out /* each [n_points][N], may be NULL */);
int sdpcut_round_csr_points_diverse(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, const double *lb, const double *ub,
                                    int64_t box_ld, int strat, int64_t sel_size, int64_t pool_size, double max_parallel,
                                    sdpcut_round_csr_t *out /* [n_points] */, sdpcut_diverse_info_t *info /* [n_points] */);

/*
 * All violated eigen-cuts of a selected set: multi-cut rounds.  A round emits ONE cut per selected index set, the eigenvector of
 * the smallest eigenvalue of [[1, x^T],[x, X]] (cut_select_qp.py:737-750); the small matrices often have several negative
 * eigenvalues, and every one of them is a valid cut.  These calls emit up to max_per_set of them per set.  The rule (DESIGN.md
 * section 5, "All violated eigen-cuts"):
 *   head            the one sdpcut_round_csr returns for (strat, sel_size) at the point: same ids, scores, n_out, n_total,
 *                   new_strat, counters (SDPCUT_OPT_EXACT_HEAD honoured, and refused, as there)
 *   entry i offers  its eigenpairs with eigenvalue < -1e-15 in ascending eigenvalue order, at most max_per_set of them (there
 *                   are at most k: the (0,0) entry is 1); equal eigenvalues keep the order of the solver's columns
 *   row             as sdpcut_cut_rows builds it from a vector: components with |v| <= 1e-15 zeroed, coefficient v_i v_j (doubled
 *                   off the diagonal) on the columns [L + i for i in set_inds] + Xarr_inds, rhs -v0^2, sense "G"
 *   walk            rows are numbered in (entry, eigenvalue) order; rows numbered >= row_quota are dropped, so the walk may end
 *                   inside an entry.  row_quota = sel_size hands the LP as many rows as a plain round at most; row_quota =
 *                   max_per_set * sel_size keeps every offered cut
 * max_per_set = 1 is sdpcut_round_csr bit for bit (the call forwards to it; n_neg is then 0 or 1: only the smallest eigenvalue
 * was looked at).  For max_per_set >= 2 all rows of an entry come from ONE full decomposition with vectors (cyclic Jacobi,
 * csrc/jacobi.h): they are an orthonormal set even inside a multiple eigenvalue, lam_min of an entry is that decomposition's
 * smallest eigenvalue, and row 0 of an entry may differ from sdpcut_round_csr's row in the last bits (another solver).
 *
 * sdpcut_round_csr_multi: strategies 1, 2, 4, 6, and 3 under SDPCUT_OPT_EXACT_SDP; vars_values NULL keeps the current point;
 * synchronous.  out->csr is the block of sdpcut_round_csr with the row arrays (row_entry, indptr, indices, values, rhs) sized for
 * row_cap = min(row_quota, max_per_set * cap) rows, plus
 *   n_neg[n_out]      violated eigenvalues of the entry (before max_per_set and before the quota)
 *   row_lam[n_rows]   the row's eigenvalue;   row_rank[n_rows]  0 for the entry's smallest eigenvalue, then 1, ...
 *   n_used            1 + row_entry[n_rows - 1], or 0 without rows;   quota_hit  1 if a row was dropped
 * row_entry ascends: a caller that keeps only the first entries (strong_only) slices a prefix.  All pointers point into the
 * handle's blocks and stay valid until the next call on the handle.
 * SDPCUT_EINVAL: max_per_set outside 1 .. SDPCUT_MULTI_MAX_PER_SET, row_quota < 1, another strategy, sel_size < 0 or a head
 * longer than 16384 entries.  SDPCUT_ESTATE: no instance, candidates or point; a round pending.
 *
 * sdpcut_cut_rows_all: the same rows for `count` LOCAL candidate ids in the caller's order (repeats allowed) at the current point;
 * no scoring, no quota.  Entry i owns rows row_ptr[i] .. row_ptr[i + 1] - 1 (row_ptr has count + 1 entries); row_lam, coef
 * [.][SDPCUT_ROW_LD] and rhs are per ROW and must hold count * max_per_set rows; cols [count][SDPCUT_ROW_LD] and ks [count] are per
 * ENTRY as in sdpcut_cut_rows (the rows of an entry share their columns).  max_per_set = 1: the rows sdpcut_cut_rows gives for the
 * entries with lam_min < -1e-15, bit for bit.  Serves strategy 5, the QCQP round's concatenated list and caller-side merges.
 *
 * Not offered in this version: multi-cut rounds together with max_parallel (sdpcut_round_csr_diverse), for batched points
 * (sdpcut_round_csr_points), for the sharded rounds (sdpcut_shard_*), and in two halves (begin / end).
 */
#define SDPCUT_MULTI_MAX_PER_SET 5
typedef struct sdpcut_round_multi {
    sdpcut_round_csr_t csr;
    int64_t row_cap;
    int64_t n_used;
    int32_t quota_hit, reserved;
    const int32_t *n_neg;
    const double *row_lam;
    const int32_t *row_rank;
} sdpcut_round_multi_t;
int sdpcut_round_csr_multi(sdpcut_handle h, const double *vars_values, int strat, int64_t sel_size, int32_t max_per_set,
                           int64_t row_quota, sdpcut_round_multi_t *out);
int sdpcut_cut_rows_all(sdpcut_handle h, int64_t count, const int64_t *idx, int32_t max_per_set, int64_t *row_ptr, double *row_lam,
                        double *coef, double *rhs, int64_t *cols, int32_t *ks);

/*
 * Cut pool: age out slack cuts, separate parked ones again.  Without it every cut of every round stays in the LP for good.  The
 * pool holds the rows a loop has added (eigen-cuts, triangle rows; any sparse row of at most SDPCUT_ROW_LD entries on the LP's
 * columns [X packed | x]), each either IN THE LP (state 0) or PARKED (state 1), in ascending order of a serial number given at add
 * time (strictly increasing, never reused).  One step at an LP point v ("Cut pool"; cutpool.py is the twin):
 *   act  = sum over the row's entries, left to right, of value * v[column]   (multiply and add separate, no contraction)
 *   norm = sqrt(sum of value^2), same order, computed once at add time
 *   d    = sense * (act - rhs)   (sense +1: a.v >= rhs, -1: a.v <= rhs; d >= 0 means satisfied)
 *   a row in the LP      age = (d > tight_tol * norm) ? age + 1 : 0; at age >= max_age it is parked with age 0 and reported in `leave`
 *   a row parked before  violated iff -d > viol_tol * norm, key (-d) / norm.  The violated rows by (key descending, serial
 *   the step             ascending): the first max_return return to the LP with age 0 and are reported in `enter` in that order,
 *                        with their rows in CSR form and their keys.  Every other parked row gets age + 1 and is DROPPED at
 *                        age >= drop_age: reported in `dropped` and removed (the rows behind it move up, order kept).
 * A row parked by a step is not examined as parked in that step.  One host wait per step.
 *
 * sdpcut_pool_create: capacity = most rows the pool ever holds at once, 1 .. SDPCUT_POOL_MAX_ROWS; there is no eviction under
 *   pressure.  Needs sdpcut_set_instance (columns are checked against nb_lifted + nb_vars); a later sdpcut_set_instance with
 *   another nb_vars makes every pool call but create / destroy fail with SDPCUT_ESTATE.  An existing pool is replaced.  Device
 *   memory: about 600 bytes per row of capacity (two sets of arrays: the compaction writes out of place).
 * sdpcut_pool_destroy: frees it (sdpcut_destroy does too); no pool is fine.
 * sdpcut_pool_add_csr: n_rows rows from host CSR arrays (row i = entries indptr[i] .. indptr[i + 1] - 1), state 0, age 0, serials
 *   *first_serial .. *first_serial + n_rows - 1.  sense may be NULL (all +1).  Refused with SDPCUT_EINVAL, the pool unchanged: an
 *   empty row, a row longer than SDPCUT_ROW_LD, a column outside [0, nb_lifted + nb_vars), a non-finite coefficient or right-hand
 *   side, a sense other than +-1, a block that would exceed the capacity.
 * sdpcut_pool_step: vars_values as in sdpcut_round_csr (NULL keeps the handle's current point; otherwise the call sets it, and a
 *   round that follows may pass NULL).  All pointers of *out point into a pinned block of the pool: valid until the next pool call.
 *   leave / dropped are in ascending serial order.  n_in_lp / n_parked count the rows after the step.
 * sdpcut_pool_get: the whole state in row order, for tests and tools: *n_rows, *next_serial and the first min(max_rows, *n_rows)
 *   entries of every array that is not NULL; cols / vals are [.][SDPCUT_ROW_LD], zero beyond a row's nnz.
 */
#define SDPCUT_POOL_MAX_ROWS 4194304
typedef struct sdpcut_pool_params {
    double tight_tol, viol_tol;
    int32_t max_age, drop_age;
    int64_t max_return;
} sdpcut_pool_params_t;
typedef struct sdpcut_pool_step {
    int64_t n_in_lp, n_parked;      /* after the step */
    int64_t n_violated;             /* violated parked rows before the cap max_return */
    int64_t n_dropped, n_leave, n_enter, enter_nnz;
    const int64_t *leave;           /* n_leave serials */
    const int64_t *enter;           /* n_enter serials, rank order */
    const int64_t *dropped;         /* n_dropped serials */
    const int32_t *enter_indptr;    /* n_enter + 1 */
    const int32_t *enter_indices;   /* enter_nnz */
    const double *enter_values;     /* enter_nnz */
    const double *enter_rhs;        /* n_enter */
    const int32_t *enter_sense;     /* n_enter */
    const double *enter_key;        /* n_enter */
} sdpcut_pool_step_t;
int sdpcut_pool_create(sdpcut_handle h, int64_t capacity);
int sdpcut_pool_destroy(sdpcut_handle h);
int sdpcut_pool_add_csr(sdpcut_handle h, int64_t n_rows, const int32_t *indptr, const int32_t *indices, const double *values,
                        const double *rhs, const int32_t *sense, int64_t *first_serial);
int sdpcut_pool_step(sdpcut_handle h, const double *vars_values, const sdpcut_pool_params_t *params, sdpcut_pool_step_t *out);
int sdpcut_pool_get(sdpcut_handle h, int64_t max_rows, int64_t *n_rows, int64_t *next_serial, int64_t *serial, int32_t *state,
                    int32_t *age, int32_t *nnz, int32_t *sense, double *rhs, double *norm, int32_t *cols, double *vals);

/*
 * The pool at tree nodes: separated at many LP points per call, read-only, and rows removed by serial -- what a GLOBAL pool needs
 * (a branch-and-cut code separates from the pool of cuts found elsewhere in the tree before it runs its separators).  The rule
 * ("Cut pool"; cutpool.py is the twin), for n_points points v_p of nb_lifted + nb_vars entries (point p at
 * points + p * point_ld):
 *   act, d = sense * (act - rhs) and norm are exactly the step's.  Row r is EXAMINED at every point iff (1 << state[r]) & state_mask
 *   (SDPCUT_POOL_SEP_LP: the rows in the LP, SDPCUT_POOL_SEP_PARKED: the parked ones; both: all rows, what a global pool uses).  An
 *   examined row is violated at p iff -d > viol_tol * norm, key (-d) / norm: the step's test and key of a parked row.  Per point:
 *   n_violated (before the cap) and the first n_rows = min(max_return, n_violated) violated rows by (key descending, serial
 *   ascending) in CSR form with their serials and keys.  max_return = 0 returns the counts only.
 * NOTHING changes: the pool (states and ages included), the handle's LP point, scores, candidate list and box are what they were.
 * One kernel launch -- a workgroup per point -- and ONE host wait per call (csrc/pool_points.hip); select_passes = 0 where every
 * violated row fitted the workgroup's list of 4096 entries, else the number of radix digit passes the selection ran (8).
 * All pointers of out[p] point into a pinned block of the pool: valid until the next pool call.  An empty pool returns zeros.
 * SDPCUT_ESTATE: no pool, a pool made for another nb_vars, a round pending.  SDPCUT_EINVAL, nothing changed: n_points outside
 * 1 .. SDPCUT_BATCH_MAX_POINTS, point_ld < nb_lifted + nb_vars, points or out NULL, state_mask 0 or with bits beyond 3, viol_tol
 * negative or not finite, max_return outside 0 .. SDPCUT_POOL_SEP_MAX_RETURN, a result block above 256 MiB (n_points slices, each
 * sized for min(max_return, rows of the pool) rows of SDPCUT_ROW_LD entries: about 272 bytes per row).
 *
 * sdpcut_pool_drop: every row whose serial is among serials[0 .. n-1] (any order; duplicates count once; serials not in the pool are
 *   ignored; n = 0 is fine) leaves the pool by the step's stable compaction: the rows behind it move up, order kept, serials are
 *   never reused.  *n_dropped (may be NULL) = the number removed.  One host wait.
 */
#define SDPCUT_POOL_SEP_LP 1u
#define SDPCUT_POOL_SEP_PARKED 2u
#define SDPCUT_POOL_SEP_MAX_RETURN 4096
typedef struct sdpcut_pool_sep {     /* one per point; pointers into a pinned block of the pool, valid until the next pool call */
    int64_t n_violated, n_rows, nnz;
    int32_t select_passes;           /* 0: every violated row fitted the workgroup's LDS list; else radix digit passes run */
    const int64_t *serial;           /* n_rows, rank order */
    const double *key;               /* n_rows, rank order */
    const int32_t *indptr;           /* n_rows + 1 */
    const int32_t *indices;          /* nnz */
    const double *values;            /* nnz */
    const double *rhs;               /* n_rows */
    const int32_t *sense;            /* n_rows */
} sdpcut_pool_sep_t;
int sdpcut_pool_separate_points(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, uint32_t state_mask,
                                double viol_tol, int64_t max_return, sdpcut_pool_sep_t *out /* [n_points] */);
int sdpcut_pool_drop(sdpcut_handle h, int64_t n, const int64_t *serials, int64_t *n_dropped);

/*
 * Dense eigen-cuts: strategy 0 of cut_select_algo, the paper's baseline (replaces __gen_dense_eigcuts, cut_select_qp.py:757-786:
 * numpy.linalg.eigh of the whole lifted matrix [[1, x^T],[x, X]] of order dim = nb_vars + 1 and the per-entry Python comprehension
 * that builds one fully dense cut for every negative eigenvalue but the largest).  Both calls need sdpcut_set_instance and a point
 * only -- no candidates, no networks (SDPCUT_ESTATE without them) -- and nb_vars <= SDPCUT_DENSE_MAX_VARS (SDPCUT_EINVAL beyond:
 * the eigensolver is one workgroup with the matrix resident in LDS, csrc/dense.hip).  Neither touches the candidate list or its
 * scores.  A round begun with sdpcut_round_csr_begin must be ended first (SDPCUT_ESTATE).
 *
 * sdpcut_dense_round: vars_values as in sdpcut_round_csr (NULL keeps the current point).  Two kernels and ONE host wait:
 *   eigvals[dim]            all eigenvalues, ascending (two-sided cyclic Jacobi; within a few ulp of ||A||_F of LAPACK's);
 *                           eigvals[0] is lambda_min of the lifted matrix -- the PSD-infeasibility of the LP point itself
 *   n_rows                  #{r < nb_vars : eigvals[r] < -1e-15} (:773-774); row r belongs to eigvals[r]
 *   cols[row_len]           [L .. L+n-1 | 0 .. L-1], the LP columns of EVERY row (:779), row_len = n + n(n+1)/2
 *   values[n_rows][row_len] [2 v0 v1 .. 2 v0 vn | v1^2, 2 v1 v2, .., vn^2] of the unit eigenvector v of eigvals[r] (:776-777);
 *                           unlike the sparse rows NO component is zeroed
 *   rhs[n_rows]             -v0^2 (:780); every row has sense "G"
 *   sweeps                  Jacobi sweeps the decomposition took
 * The pointers point into the handle's pinned host block (written by the device): valid until the next call on the handle.
 * With SDPCUT_OPT_TIMING, sdpcut_last_timing reports ms[0] = the eigensolver and (option value 2) ms[1] = the row assembly.
 *
 * sdpcut_dense_eig: the decomposition alone at the current point.  eigvals[dim] ascending; evecs (may be NULL) [dim][dim] with
 * evecs[i][j] = component i of the eigenvector of eigvals[j] (numpy's column convention).  Caller-owned buffers.
 */
#define SDPCUT_DENSE_MAX_VARS 127
typedef struct sdpcut_dense_round {
    int32_t dim, n_rows, sweeps, reserved;   /* dim = nb_vars + 1 */
    int64_t row_len;                         /* n + n(n+1)/2 */
    const double *eigvals;                   /* dim, ascending; row r belongs to eigvals[r] */
    const int32_t *cols;                     /* row_len, shared by all rows */
    const double *values;                    /* [n_rows][row_len] */
    const double *rhs;                       /* n_rows */
} sdpcut_dense_round_t;
int sdpcut_dense_round(sdpcut_handle h, const double *vars_values, sdpcut_dense_round_t *out);
int sdpcut_dense_eig(sdpcut_handle h, double *eigvals, double *evecs);

/*
 * The same round over candidate shards (one handle per GPU, SURVEY 8 e): the two device-side
 * halves around the single all-gather the caller performs (torch.distributed / RCCL).
 *
 * sdpcut_shard_head_device: enqueue, WITHOUT host synchronisation, this shard's head of the
 * ranking (strat 1, 2, SDPCUT_PART_STRONG or SDPCUT_PART_COMBALL) into one packed device record of
 * 8 + fields * count int64 words (fields = 3 for SDPCUT_PART_COMBALL, else 2)
 *     [list length, nb_violated, nb_positive, entries written, void flag, 0, 0, 0 |
 *      count scores (fp64 bits) | count GLOBAL ids | (fields = 3) count secondary keys = obj_improve (fp64 bits)]
 * padded with (-inf, INT64_MAX, -inf); 1 <= count <= 16384.  Measures the strategy needs and sdpcut_score has
 * not computed since the last sdpcut_set_point are scored by this call (a sharded round is set_point,
 * shard_head, all-gather, shard_finish); when none of them has been, the score kernels also prepare the
 * selection's first radix digit (SDPCUT_OPT_FUSE_KEYS).
 *
 * sdpcut_shard_finish_enqueue / sdpcut_shard_finish_wait: d_allrec holds the `world` records in rank order
 * (`fields` as above).  Enqueue merges them by (score descending, [secondary descending,] id ascending) -- the order
 * of the reference's stable sorts on one list (cut_select_qp.py:601, :625, :653) --, keeps the first sel_size entries
 * and produces the eigen-cut rows of those that belong to THIS shard (the others: ks = 0, lam_min = NaN), all stored
 * by the device into the handle's pinned block; wait returns the block (layout below) once it is complete -- the
 * round's only host synchronisation.  Several handles may have their halves enqueued before the first wait.
 * sdpcut_shard_finish_round*: the two calls in one, fields = 2.  headers [world][8] are the record headers (the
 * caller sums them); entries beyond the summed list length are pads.
 */
int sdpcut_shard_head_device(sdpcut_handle h, int strat, int64_t count, void *d_record);
/* pitch_words: distance between the records of consecutive ranks in d_allrec, in int64 words (0 = the record's own length:
 * one list per gathered buffer); larger when the records of several lists travel in one all-gather (the QCQP round's two
 * covers: d_allrec then points at this list's record of rank 0 inside the buffer). */
int sdpcut_shard_finish_enqueue(sdpcut_handle h, int32_t world, int64_t count, int32_t fields, const void *d_allrec,
                                int64_t pitch_words, int64_t sel_size, int32_t coef_ld);
/* compact_own != 0: block as sdpcut_shard_finish_round_own, *n_own = rows of this shard; 0: as sdpcut_shard_finish_round_view */
int sdpcut_shard_finish_wait(sdpcut_handle h, int32_t compact_own, const void **block, int64_t *n_own);
int sdpcut_shard_finish_round(sdpcut_handle h, int32_t world, int64_t count,
                              const void *d_allrec, int64_t sel_size, int32_t coef_ld,
                              int64_t *headers_out, int64_t *idx_out, double *score_out,
                              double *lam_min, double *coef, double *rhs, int32_t *ks);
/* Zero-copy form (see sdpcut_select_round_view): *block = the handle's pinned host block
 *     int64 headers[world][8] | int64 idx[sel_size] | double score[sel_size] |
 *     double lam_min[sel_size] | double rhs[sel_size] | double coef[sel_size][coef_ld] |
 *     int32 ks[sel_size]
 * written by the device, valid until the next call on the handle. */
int sdpcut_shard_finish_round_view(sdpcut_handle h, int32_t world, int64_t count,
                                   const void *d_allrec, int64_t sel_size, int32_t coef_ld,
                                   const void **block);
/* Same block, but the *n_own rows of THIS shard are moved to the front of lam_min / rhs / coef /
 * ks (keeping head order) and an array  int32 pos[sel_size]  is appended behind ks: pos[j] = the
 * position in the merged head of own row j.  idx / score stay the full replicated head. */
int sdpcut_shard_finish_round_own(sdpcut_handle h, int32_t world, int64_t count,
                                  const void *d_allrec, int64_t sel_size, int32_t coef_ld,
                                  const void **block, int64_t *n_own);

/*
 * Batched twin of _get_eigendecomp (cut_select_qp.py:788-797) for explicit sub-matrices:
 * x_rho [count][k], X_rho [count][k(k+1)/2] (upper triangle, row-major).  Writes ascending
 * eigenvalues [count][k+1] and, if evecs != NULL, eigenvectors [count][k+1][k+1] with
 * evecs[c][i][j] = component i of eigenvector j (numpy's column convention).
 */
int sdpcut_eig_batch(sdpcut_handle h, int k, int64_t count, const double *x_rho,
                     const double *X_rho, double *eigvals, double *evecs);

/* Batched raw MLP forward: inputs [count][d_in] -> out [count] (the NNs.so call, batched). */
int sdpcut_nn_batch(sdpcut_handle h, int k, int64_t count, const double *inputs, double *out);

/*
 * Batched exact solve of the small SDP above on explicit inputs (the label generator for a user's own networks -- the targets
 * sdpcut_set_network's MLPs are trained on -- and the window on the certificate): inputs [count][k(k+3)/2] = [x | Q_slice], the
 * layout of sdpcut_nn_batch.  value [count] = certified LOWER bound on p*, gap [count] = upper - lower; optional (may be NULL):
 * lam [count][k] the dual point, Y [count][k(k+1)/2] the primal point (upper triangle, row-major), iters [count] iterations taken.
 * Needs nothing but the handle.
 */
int sdpcut_sdp_batch(sdpcut_handle h, int k, int64_t count, const double *inputs, double *value, double *gap, double *lam,
                     double *Y, int32_t *iters);

/*
 * Training a network of one's own (the step between sdpcut_sdp_batch's labels and sdpcut_set_network): loss and gradient of a
 * tansig MLP over a data set resident on the device.  The optimiser runs on the host (networks.py: train -- scaled conjugate
 * gradient) and calls sdpcut_train_loss_grad twice per iteration.
 *
 * sdpcut_train_set_data copies `count` samples of size k to the device: inputs [count][k(k+3)/2] = [x | Q_slice], the layout of
 * sdpcut_nn_batch, and targets [count] (e.g. the values of sdpcut_sdp_batch).  One set per candidate size; a new call replaces
 * it, count = 0 drops it.  The set belongs to the handle and is independent of instance, candidates, point and networks.
 *
 * sdpcut_train_loss_grad: k, n_layers, widths, params, n_params are EXACTLY the packing of sdpcut_set_network, refused where and
 * as that call refuses them.  In normalised units -- what MATLAB's mse performance minimises --
 *     x_n = (x - xoffset) gain + ymin,  a_l = tansig(W_l a_(l-1) + b_l) for the hidden layers,  y_n = W_out a + b_out,
 *     t_n = (t - y_xoffset) y_gain + y_ymin,      *loss = (1 / count) sum (y_n - t_n)^2   over samples [first, first + count)
 * with tansig(n) = 2 / (1 + exp(-2n)) - 1 and NO input clamp (SDPCUT_INPUT_CLAMP is an inference matter).  grad (may be NULL:
 * forward only) receives d loss / d(W, b) of every layer in the order of params: n_params - (2 d_in + 1 + 3) doubles -- the
 * mapping constants are data, not parameters.  fp64 throughout, the matrix products on v_mfma_f64_16x16x4_f64; the partial
 * gradients of the workgroups are added in a fixed order and nothing is accumulated atomically: two calls with the same arguments
 * return the same bits, and *loss is the same with and without a gradient.
 * Memory: a call keeps a workspace of (min(ceil(count / 16), 2 x compute units) + 1) x (n_params - 2 d_in - 3) + n_params doubles
 * on the handle -- one row of partial sums per workgroup, 57 MB for the k = 5 network with four hidden layers of 64 on 256 compute
 * units.  It grows to the largest call's need, is written and read once per evaluation and is freed with the handle.
 * Needs nothing but the handle and the data: SDPCUT_ESTATE before sdpcut_train_set_data for this k and while a round begun with
 * sdpcut_round_csr_begin is pending; SDPCUT_EINVAL for a bad k, a range outside the set or an n_params that does not match.
 */
int sdpcut_train_set_data(sdpcut_handle h, int k, int64_t count, const double *inputs, const double *targets);
int sdpcut_train_loss_grad(sdpcut_handle h, int k, int n_layers, const int32_t *widths, const double *params, int64_t n_params,
                           int64_t first, int64_t count, double *loss, double *grad);

/* Timing of the last sdpcut_score / sdpcut_rank (HIP events on the handle's stream).
 * SDPCUT_OPT_TIMING = 1: events around the score kernels only; = 2: also around the ranking.
 * ms[0] = score kernels, ms[1] = rank (-1 when not recorded). */
int sdpcut_last_timing(sdpcut_handle h, double *ms, int n);

/*
 * Semidefinite vertex cover P^E_dim (replaces the index-set enumeration of
 * _get_sdp_vertex_cover, cut_select_qp.py:399-524, ch_ext = 0): every clique of size `dim`
 * of the sparsity graph plus every maximal clique of size 2..dim-1, in the reference's order.
 * adjacency is [nb_vars][nb_vars] bytes (non-zero = edge; symmetrised, diagonal ignored).
 * Writes at most max_out rows of set_inds_out [.][5] (padded with -1) / ks_out and always the
 * full count (call with max_out = 0 to size the arrays; the reference bails out at 4e6,
 * _THRES_MAX_SUBS).  Host function, no handle needed.
 */
int sdpcut_enumerate_cover(int32_t nb_vars, const uint8_t *adjacency, int32_t dim, int64_t max_out,
                           int32_t *set_inds_out, int32_t *ks_out, int64_t *count_out);

/*
 * Host twin of sdpcut_set_candidates_cover_ch at dim 3: ch_ext = 0 / 1 / -1 are sdpcut_enumerate_cover on adjacency_orig /
 * adjacency_ext / the complete graph, ch_ext = 2 is bar(P*_3).  Per edge (i1,i2) of the EXTENDED graph, in lexicographic order:
 * every forward triangle (i3 > i2 adjacent to both in the extended graph) with at least 2 of its 3 edges in the ORIGINAL graph;
 * if there is none and no smaller i3 != i1 closes such a triangle and (i1,i2) is an original edge, the pair.  Outputs as in
 * sdpcut_enumerate_cover.  An adjacency the mode does not read may be NULL.  Host function, no handle needed.
 */
int sdpcut_enumerate_cover_ch(int32_t nb_vars, const uint8_t *adjacency_ext, const uint8_t *adjacency_orig, int32_t ch_ext,
                              int64_t max_out, int32_t *set_inds_out, int32_t *ks_out, int64_t *count_out);

/*
 * Chordal extension of a sparsity pattern by the elimination game (replaces chompack's symbolic factorisation,
 * cut_select_qp.py:386-396).  adjacency: [nb_vars][nb_vars] bytes, symmetrised, diagonal ignored; 2 <= nb_vars <= 1024
 * (SDPCUT_EINVAL otherwise).  For each vertex v of the order, the not-yet-eliminated neighbours of v in the current filled graph
 * become a clique, then v is eliminated.
 *   ext_out   [nb_vars][nb_vars] bytes: the original edges plus the fill, symmetric, zero diagonal -- a chordal graph;
 *   order_out [nb_vars]: the order used, a perfect elimination ordering of ext_out;
 *   fill_out  the number of fill edges.
 * order_in (may be NULL) must be a permutation of 0..nb_vars-1 (SDPCUT_EINVAL otherwise): a caller who holds the reference's AMD
 * permutation gets the reference's pattern exactly.  With NULL the order is greedy minimum degree on the elimination graph: at
 * each step the not-yet-eliminated vertex with the fewest not-yet-eliminated neighbours in the current filled graph, ties to the
 * lowest index.  This is NOT cvxopt's AMD: cover sizes can differ from the published nb_subproblems.
 * Host function, no handle and no GPU needed.
 */
int sdpcut_chordal_extension(int32_t nb_vars, const uint8_t *adjacency, const int32_t *order_in, uint8_t *ext_out,
                             int32_t *order_out, int64_t *fill_out);

/*
 * Triangle inequalities (SURVEY.md section 8 f row 3; cut_select_qp.py:799-863).
 * sdpcut_tri_preprocess (replaces __preprocess_triangle_ineq, :799-822): keeps the triples
 *   i1<i2<i3 with at least two of their three edges in the sparsity graph (adjacency as in
 *   sdpcut_enumerate_cover), lexicographic; needs sdpcut_set_instance.  sdpcut_tri_get_triples
 *   copies them out ([T][3], density 2 or 3 per triple).
 * sdpcut_tri_separate (replaces the scan and sort of __separate_and_add_triangle, :829-842):
 *   at the current LP point computes the four violations of every triple, keeps those
 *   >= 1e-7, orders them by (density desc, violation desc), ties in entry order, and returns
 *   the first max_out as entry ids 4*triple + type with their violations.  *n_violated is the
 *   length of the full list (the caller derives the number of cuts from it, :844-845).
 */
int sdpcut_tri_preprocess(sdpcut_handle h, const uint8_t *adjacency, int64_t *n_triples);
int sdpcut_tri_get_triples(sdpcut_handle h, int32_t *triples_out, uint8_t *density_out);
int sdpcut_tri_separate(sdpcut_handle h, int64_t max_out, int64_t *entry_out, double *viol_out,
                        int64_t *n_violated, int64_t *n_written);

/*
 * Triangle rounds with the rows assembled on the device, at the root and at tree nodes (DESIGN.md section 5 "Triangle inequalities
 * at nodes"; numpy twin: sdpcutsel_via_nn_amd/triangles.py).
 * sdpcut_tri_round_csr: the separation of sdpcut_tri_separate followed by the rows of the selected entries, as one CSR block in a
 *   pinned host block of the handle; one host wait.  vars_values: the LP point [X packed | x] (sdpcut_set_point is part of the
 *   call), or NULL to keep the current one.  0 <= max_out <= 16384.  Needs sdpcut_tri_preprocess (SDPCUT_ESTATE without).
 *   All pointers of *out point INTO the handle's block: valid until the next call on the handle, never freed by the caller.
 *     n_violated  length of the full list of violated entries;  n_rows = min(max_out, n_violated)
 *     entry [n_rows], viol [n_rows]   what sdpcut_tri_separate returns: 4 * triple + type, ranked (density 3 first, violation
 *                                     descending, entry ascending)
 *     rhs [n_rows], indptr [n_rows + 1], indices / values [nnz = indptr[n_rows]]   row r, sense >=, in the columns of vars_values:
 *                                     X_ab, X_ac, X_bc, then the x columns in ascending variable order
 *   Without a node box row r is the row the reference builds (:847-861): 4 non-zeros +-1 and rhs 0 for types 0 .. 2, 6 non-zeros and
 *   rhs -1 for type 3.  With a node box (sdpcut_set_box) the call separates the triangle inequalities OF THE BOX: the violations
 *   are those of the box tables x' = (x - l) / d, X' (sdpcut_get_box_tables; violated: >= 1e-7 in those units; density is the
 *   original pattern's), and row r is that facet written in the original (x, X) -- valid on the box, where the unit-box facet is
 *   weaker -- with up to 3 x columns and a right-hand side; a coefficient that is exactly zero is dropped.  On the unit box every
 *   byte equals the call without a box.
 * sdpcut_tri_round_csr_points: the same at n_points LP points (row p of `points`, point_ld >= L + n doubles apart; 1 <= n_points <=
 *   SDPCUT_BATCH_MAX_POINTS) in one call with one host wait; lb / ub: both NULL, or [n_points][n] each -- the node box of every
 *   point, checked by sdpcut_set_box's rule.  out[p] is, bit for bit, what sdpcut_set_box(lb[p], ub[p]) (or no box) followed by
 *   sdpcut_tri_round_csr(points[p], max_out) returns; its pointers point into the handle's pinned batch block (slice p, padded to
 *   64 bytes).  One-wait route (SDPCUT_STAT_TRI_POINTS_FAST counts its points): max_out <= 4096 and the per-point tables within
 *   256 MB -- one workgroup per point selects by radix over recomputed keys, sorts its head and emits its rows; everything else
 *   runs the single-point call per point inside the call.  Refused (SDPCUT_ESTATE) while the handle has a box of its own; leaves
 *   the handle without a current point and without a box.
 */
typedef struct sdpcut_tri_csr {
    int64_t cap;                    /* min(max_out, 4 T): entries the block has room for */
    int64_t n_rows, n_violated, nnz;
    const int64_t *entry;
    const double *viol;
    const int32_t *indptr;
    const int32_t *indices;
    const double *values;
    const double *rhs;
} sdpcut_tri_csr_t;
int sdpcut_tri_round_csr(sdpcut_handle h, const double *vars_values, int64_t max_out, sdpcut_tri_csr_t *out);
int sdpcut_tri_round_csr_points(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, const double *lb,
                                const double *ub, int64_t max_out, sdpcut_tri_csr_t *out);

/*
 * Node evaluation: what a tree node needs after its LP solves and separation rounds, at n_points LP points in one launch with one
 * host wait (DESIGN.md section 5 "Node evaluation"; numpy twin, equal bit for bit: sdpcutsel_via_nn_amd/nodeeval.py).
 * The objective is the handle's LP objective (sdpcut_set_objective) over [X packed | x]: a_ij = obj[pos(i, j)] for i <= j,
 * c_i = obj[L + i], f(x) = sum_{i <= j} a_ij x_i x_j + sum_i c_i x_i.  Per point p, with its box lb[p], ub[p] or the unit box:
 *   projection   x <- min(max(x, l), u); everything below uses this x and the point's own X
 *   f_point      f at the projected x
 *   local search Gauss-Seidel coordinate descent inside the box, i ascending, at most max_sweeps sweeps: s = c_i + sum_{j != i}
 *                a_ij x_j, a = a_ii; a > 0: t = clamp(-s / (2 a), l_i, u_i), else t = the endpoint with the smaller
 *                phi(t) = (a t + s) t, a tie going to l_i; x_i <- t only if phi(t) < phi(x_i) strictly; a sweep without a move
 *                ends the search (it is counted in `sweeps`).  x_local [n], f_local = f(x_local), sweeps, moves
 *   branching    candidates: u_i - l_i >= 4 SDPCUT_BOX_MIN_WIDTH.  branch_rule 0: g_i = X_ii - x_i^2; 1: g_i = sum_j |a_ij|
 *                |X_ij - x_i x_j|, j = i included.  branch_var = the largest g, lowest index on ties (-1 and score 0 without a
 *                candidate), branch_score = that g, branch_val = clamp(x_i, l_i + m, u_i - m), m = max(rho (u_i - l_i),
 *                SDPCUT_BOX_MIN_WIDTH), then moved by single ulps where the rounding of l_i + m or u_i - m would leave a child
 *                narrower than SDPCUT_BOX_MIN_WIDTH: both children keep a width sdpcut_set_box accepts
 * The orders of the sums are documented in csrc/node_eval.hip; nothing is contracted.
 * READ-ONLY: the handle's point, scores, box, pending round and pool stay as they were; the call is allowed while a box is set (it
 * does not use it) and between the halves of a round.  Needs sdpcut_set_instance and sdpcut_set_objective (SDPCUT_ESTATE without);
 * the first call after a sdpcut_set_objective builds the objective's dense n x n table on the device (one more launch in front of
 * the evaluation, the same single wait) and the handle keeps it until the objective changes.
 * SDPCUT_EINVAL, the handle unchanged: n_points outside 1 .. SDPCUT_BATCH_MAX_POINTS, more than 1024 variables, point_ld < L + n,
 * a non-finite entry of a point or a bound, only one of lb / ub, a bound outside 0 <= l < u <= 1, max_sweeps < 0, branch_rule not
 * 0 or 1, rho outside (0, 0.5].  Widths below SDPCUT_BOX_MIN_WIDTH are NOT refused: such a variable is never a candidate.
 * x_local points INTO a pinned block of the handle (slice p: a 64-byte header, then n doubles, padded to 64 bytes): valid until
 * the next call of this function on the handle.  SDPCUT_STAT_NODE_EVAL_POINTS counts the points evaluated.
 */
typedef struct sdpcut_node_eval {
    double f_point, f_local;
    double branch_score, branch_val;
    int32_t sweeps, moves;
    int32_t branch_var, reserved;
    const double *x_local;          /* [n] */
} sdpcut_node_eval_t;
int sdpcut_node_eval_points(sdpcut_handle h, int32_t n_points, const double *points, int64_t point_ld, const double *lb /* [n_points][n] */,
                            const double *ub /* [n_points][n] */, int32_t max_sweeps, int32_t branch_rule, double rho,
                            sdpcut_node_eval_t *out /* [n_points] */);

/* Self-test hook: multiplies A[16x4] * B[4x16] with v_mfma_f64_16x16x4_f64 using the
 * fragment maps the MLP kernel assumes; C row-major [16][16]. */
int sdpcut_mfma_probe(sdpcut_handle h, const double *A, const double *B, double *C);

/*
 * The reference's own FFI (neural_net_{2,3,4,5}D, NNs_initialize, NNs_terminate; cut_select_qp.py:297-303) is exported by the
 * sibling library libsdpcut_nns.so -- include/sdpcut_nns.h -- which binds to this one privately (sdpcut_create,
 * sdpcut_set_builtin_networks, sdpcut_nn_batch).  Until round 4 this library exported the six names itself.
 */

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SDPCUT_H */
