// Internal to the top-k selection: the launchers through which topk.hip (host only) starts the kernels of the route files.
// No kernel is referenced from another translation unit.  Grids and template arguments come from the plan (topk_route.h);
// the launchers enqueue on h->stream and leave hipGetLastError to the caller.
#pragma once
#include "topk_dev.h"

// what a selection reads and where its head goes
struct TkJob {
    TopkWs *ws;
    int mode;                     // TK_MODE_*
    int64_t n, k, sel;            // candidates, head, sel_size of the combined strategy (COMBAUTO)
    const double *eig, *obj;      // the scores (NULL: not scored / keys precomputed in h->d_key_a)
    int64_t base;                 // added to the emitted indices
    double score_add;
    int64_t *d_idx_out;
    double *d_score_out;
    int raw;                      // see tk_mergerank_big_kernel
    int64_t emit_limit;
    const double *tie_obj = nullptr;   // obj_improve the sort tail orders equal keys by (modes with a tie key); NULL: the handle's scores
};

// topk_passes.hip: the key passes, the fused kernel (TK_ROUTE_ONFLY / TK_ROUTE_COOP / TK_ROUTE_FUSED), the launch per digit
void tk_keys_launch(sdpcut_ctx *h, const TkPlan &p, const TkJob &j);         // tk_keys_kernel -> h->d_key_a
void tk_prekeys_launch(sdpcut_ctx *h, const TkPlan &p, const TkJob &j);      // tk_prekeys_kernel over h->d_key_a
int tk_refine_launch(sdpcut_ctx *h, const TkPlan &p, const TkJob &j);
void tk_hist_launch(sdpcut_ctx *h, const TkPlan &p, const TkJob &j);         // tk_hist_kernel x 7
int tk_refine_coresident(sdpcut_ctx *h, int64_t *coresident);               // workgroups of tk_refine_kernel the device holds at once
// topk_compact.hip: tk_count_kernel, tk_write_kernel behind tk_hist_launch (TK_ROUTE_DIGITS)
void tk_compact_launch(sdpcut_ctx *h, const TkPlan &p, const TkJob &j);
// topk_small.hip: TK_ROUTE_SMALLSORT / TK_ROUTE_SMALLSEL / TK_ROUTE_SMALL
void tk_small_launch(sdpcut_ctx *h, const TkPlan &p, const TkJob &j);
// topk_sort.hip: the sort tail
void tk_sort_launch(sdpcut_ctx *h, const TkPlan &p, const TkJob &j);
