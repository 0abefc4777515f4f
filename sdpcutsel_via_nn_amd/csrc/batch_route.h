// Batched rounds (sdpcut_round_csr_points, sdpcut_round_csr_points_diverse; points.hip): which way a batch of LP points over one
// candidate list goes, and the layout of the pinned block its results come back in.  Plain C++, no HIP: the host code (points.hip),
// tests/test_batch_points_cpu.py and tests/test_diverse_points_cpu.py (which compile this header alone) read both here and nowhere
// else.  Of the filtered batch, the combined strategy (4) with a pool longer than its quota loops: see batch_route_diverse.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "round_layout.h"
#include "topk_route.h"

enum BatchRoute {
    BATCH_FAST = 1,   // one point copy, one score launch, one selection launch (a workgroup per point), one row assembly, one wait
    BATCH_LOOP = 2    // the single-point round once per point inside the call, each result copied into the point's slice
};

// The selection mode a batched round of strategy strat runs in (the combined strategy resolves its regime on the device, per
// point, from the strong count the score launch leaves); 0: the strategy is not served.
static inline int batch_mode(int strat)
{
    return strat == SDPCUT_STRAT_FEAS ? TK_MODE_FEAS : strat == SDPCUT_STRAT_OPT ? TK_MODE_OPT : strat == SDPCUT_STRAT_COMB ? TK_MODE_COMBAUTO : 0;
}

// N candidates, a head of cap = min(sel_size, N) entries.  BATCH_FAST exactly when tk_route sends a fresh selection of this list
// to the one-workgroup select-sort-emit kernel (TK_ROUTE_SMALLSORT) and nothing asks for more than it gives: reference-exact
// heads (SDPCUT_OPT_EXACT_HEAD) re-rank a band of the head, a shard (global base != 0) writes a record behind it.  cap == 0 (the
// single-point code reports the ranking's length and the strategy switch without a selection) is refused by tk_route: loop.
static inline int batch_route(int64_t N, int64_t cap, int strat, bool exact_head, bool shard)
{
    const int mode = batch_mode(strat);
    if (!mode || exact_head) return BATCH_LOOP;
    TkRouteIn in;
    in.n = N;
    in.k = cap;
    in.mode = mode;
    in.stage = mode == TK_MODE_COMBAUTO ? 1 : 0;      // the strong count is there; the selection builds its own keys
    in.shard_rec = shard;
    const TkPlan p = tk_route(in);
    return (p.err == 0 && p.route == TK_ROUTE_SMALLSORT) ? BATCH_FAST : BATCH_LOOP;
}

// A boxed batch (sdpcut_round_csr_points_boxed): every point has a Q' [L] and a transformed point [L + n] of its own on the device,
// n_points (2 L + n) doubles.  n = 125 at 256 points is 33 MB; the budget only keeps a large-n instance from allocating gigabytes.
#define BATCH_BOX_BUDGET_BYTES ((int64_t)256 << 20)
static inline int64_t batch_box_table_bytes(int64_t nb_vars, int64_t n_points)
{
    const int64_t L = nb_vars * (nb_vars + 1) / 2;
    return n_points * (2 * L + nb_vars) * 8;
}

// BATCH_FAST under batch_route's conditions plus one: the box tables fit the budget.  Everything else loops -- sdpcut_set_box and
// the single-point round once per point inside the call.
static inline int batch_route_boxed(int64_t N, int64_t cap, int strat, bool exact_head, bool shard, int64_t nb_vars, int64_t n_points)
{
    if (batch_route(N, cap, strat, exact_head, shard) != BATCH_FAST) return BATCH_LOOP;
    return batch_box_table_bytes(nb_vars, n_points) <= BATCH_BOX_BUDGET_BYTES ? BATCH_FAST : BATCH_LOOP;
}

// The filtered batch (sdpcut_round_csr_points_diverse): strategies 1, 2, 4 and 6 -- strategy 6 selects as strategy 2 does, on the
// efficacy score rows.  0: not served.  (batch_mode keeps refusing 6: the plain batched round does not serve it.)
static inline int batch_mode_diverse(int strat)
{
    return strat == SDPCUT_STRAT_EFF ? TK_MODE_OPT : batch_mode(strat);
}

// the largest pool whose rows, pair bits and index sets fit the LDS of the one workgroup that filters a point (diverse.hip:
// div_points_kernel); also the longest head the one-workgroup selection emits (TK_TILE)
#define BATCH_DIVERSE_MAX_POOL 512

// N candidates, quota sel_size, pool_size entries of the ranking walked.  BATCH_FAST exactly when
//   N <= 4096, pool = min(pool_size, N) in 1 .. BATCH_DIVERSE_MAX_POOL,
//   tk_route sends a fresh selection of (N, k = pool) in the strategy's mode to TK_ROUTE_SMALLSORT,
//   reference-exact heads are off and the list has no shard base,
//   and the one-workgroup selection with k = pool gives the head sdpcut_rank(strat, sel_size, max_out = pool) gives.
// The last holds for strategies 1, 2 and 6 whatever sel_size is: their rankings do not depend on it.  It does NOT hold for the
// combined strategy (4) when min(sel_size, N) < pool: its quota stays sel_size, so in the strong regime the scan stops after sel_size
// strong candidates and the entries behind them are the unvisited rest of the list, which the selection (a top-k of the strong
// class) does not produce.  Strategy 4 with min(sel_size, N) < pool therefore LOOPS; with min(sel_size, N) == pool it is the
// selection of the plain batched round.
static inline int batch_route_diverse(int64_t N, int64_t sel_size, int64_t pool_size, int strat, bool exact_head, bool shard)
{
    const int mode = batch_mode_diverse(strat);
    if (!mode || exact_head || shard) return BATCH_LOOP;
    const int64_t pool = pool_size < N ? pool_size : N, sel = sel_size < N ? sel_size : N;
    if (N > TK_SMALLSORT_N || pool < 1 || pool > BATCH_DIVERSE_MAX_POOL || sel < 1) return BATCH_LOOP;
    if (strat == SDPCUT_STRAT_COMB && sel < pool) return BATCH_LOOP;
    TkRouteIn in;
    in.n = N;
    in.k = pool;
    in.mode = mode;
    in.stage = mode == TK_MODE_COMBAUTO ? 1 : 0;
    in.shard_rec = shard;
    const TkPlan p = tk_route(in);
    return (p.err == 0 && p.route == TK_ROUTE_SMALLSORT) ? BATCH_FAST : BATCH_LOOP;
}

// ... with a box per point: plus the box tables fit the budget (strategies 1 and 6 read no box table and need none)
static inline int batch_route_diverse_boxed(int64_t N, int64_t sel_size, int64_t pool_size, int strat, bool exact_head, bool shard,
                                            int64_t nb_vars, int64_t n_points)
{
    if (batch_route_diverse(N, sel_size, pool_size, strat, exact_head, shard) != BATCH_FAST) return BATCH_LOOP;
    if (strat == SDPCUT_STRAT_FEAS || strat == SDPCUT_STRAT_EFF) return BATCH_FAST;
    return batch_box_table_bytes(nb_vars, n_points) <= BATCH_BOX_BUDGET_BYTES ? BATCH_FAST : BATCH_LOOP;
}

// The batch block: n_points slices of `slice` bytes, slice p at offset p * slice.  A slice is one CSR round block (csr_layout:
// 128 bytes of header, then the arrays) padded to a multiple of 64 bytes, so that every point's header starts a cache line of
// its own.
struct BatchLayout { size_t slice, bytes; };
static inline BatchLayout batch_layout(int64_t cap, int ld, int n_points)
{
    BatchLayout y;
    y.slice = (csr_layout(cap, ld).bytes + 63) & ~(size_t)63;
    y.bytes = y.slice * (size_t)n_points;
    return y;
}
static inline size_t batch_point_offset(const BatchLayout &y, int p) { return y.slice * (size_t)p; }
