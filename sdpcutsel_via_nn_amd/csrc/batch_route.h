// Batched rounds (sdpcut_round_csr_points, points.hip): which way a batch of LP points over one candidate list goes, and the
// layout of the pinned block its results come back in.  Plain C++, no HIP: the host code (points.hip) and
// tests/test_batch_points_cpu.py (which compiles this header alone) read both here and nowhere else.
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
