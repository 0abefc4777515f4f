// All violated eigen-cuts of a selected set (include/sdpcut.h: sdpcut_round_csr_multi, sdpcut_cut_rows_all; the rule is DESIGN.md
// section 5 "All violated eigen-cuts", multicut.py its numpy twin).  A plain round emits one row per head entry (rows.hip); here an
// entry emits one row per violated eigenvalue, up to max_per_set of them, all from ONE Jacobi decomposition with vectors, and a row
// quota ends the walk -- inside an entry if it falls there.
//   multi_csr_kernel       the CSR assembly of a ranked head, in head order like round_csr_body (rows.hip), several rows per entry
//   cut_rows_all_kernel    padded rows of an explicit id list, one lane per entry: no quota, no look-back
// The gather, the row of an eigenvector, the look-back across workgroups and the completion word are rows_dev.h's, shared with
// the plain round's kernels; so are the handle's ticket and look-back words (rows.hip: ensure_round_sync) and the host's
// launch-wait-retry rule (round.hip: csr_assemble_wait).  The head comes from sdpcut_rank_device, as the diverse round's does.
#include <cstring>
#include <new>
#include <vector>

#include "common.h"
#include "rows_dev.h"
#include "topk_route.h"

#define MULTI_DMAX (SDPCUT_MAX_K + 1)

// The decomposition of one entry, padded to the largest order so that what follows the size switch is one piece of code.  Every
// index is a compile-time constant (jacobi.h: runtime-indexed arrays would go to scratch).
struct MultiEig {
    double v[MULTI_DMAX][MULTI_DMAX];   // v[i][j] = component i of the eigenvector of lam[j] (solver's column order); 0 beyond the order
    double lam[MULTI_DMAX];
    int rk[MULTI_DMAX];                 // position of column j in ascending eigenvalue order, equal eigenvalues by column; 99 beyond the order
    int n_neg;                          // eigenvalues < -1e-15
    double lam_min;
};

template <int K>
__device__ __forceinline__ void multi_decompose(const int32_t *s5, const double *vars, int32_t nv, int64_t L, MultiEig &E,
                                                int64_t (&cl)[SDPCUT_ROW_LD])
{
    constexpr int M = K * (K + 1) / 2;
    constexpr int D = K + 1;
    double x[K], X[M];
    gather_lifted<K>(s5, vars, nv, L, x, X, cl);
    double a[D][D], v[D][D];
    fill_lifted<K>(a, x, X);
    jacobi_eig<D, true>(a, v);
    E.n_neg = 0;
    E.lam_min = a[0][0];
#pragma unroll
    for (int j = 0; j < MULTI_DMAX; ++j) {
        E.lam[j] = j < D ? a[j < D ? j : 0][j < D ? j : 0] : 0.0;
#pragma unroll
        for (int i = 0; i < MULTI_DMAX; ++i) E.v[i][j] = (i < D && j < D) ? v[i < D ? i : 0][j < D ? j : 0] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < MULTI_DMAX; ++j) {
        int r = 0;
#pragma unroll
        for (int i = 0; i < MULTI_DMAX; ++i)
            if (i < D && j < D && i != j) r += (E.lam[i] < E.lam[j] || (E.lam[i] == E.lam[j] && i < j)) ? 1 : 0;
        E.rk[j] = j < D ? r : 99;
        if (j < D) {
            E.n_neg += E.lam[j] < SDPCUT_NEG_EIGVAL ? 1 : 0;
            E.lam_min = E.lam[j] < E.lam_min ? E.lam[j] : E.lam_min;
        }
    }
}

// the eigenpair at position r of the ascending order
__device__ __forceinline__ double multi_pick(const MultiEig &E, int r, double (&ev)[MULTI_DMAX])
{
    double lam = 0.0;
#pragma unroll
    for (int i = 0; i < MULTI_DMAX; ++i) ev[i] = 0.0;
#pragma unroll
    for (int j = 0; j < MULTI_DMAX; ++j) {
        const bool hit = E.rk[j] == r;
        lam = hit ? E.lam[j] : lam;
#pragma unroll
        for (int i = 0; i < MULTI_DMAX; ++i) ev[i] = hit ? E.v[i][j] : ev[i];
    }
    return lam;
}

// the two size-templated steps for a size known at run time
__device__ __forceinline__ void multi_decompose_k(int k, const int32_t *sp, const double *vars, int32_t nv, int64_t L, MultiEig &E,
                                                  int64_t (&cl)[SDPCUT_ROW_LD])
{
    CALL_FOR_SET_SIZE(k, multi_decompose, sp, vars, nv, L, E, cl);
}
__device__ __forceinline__ void multi_row_k(int k, const double (&ev)[MULTI_DMAX], double (&co)[SDPCUT_ROW_LD], double &rhs)
{
    CALL_FOR_SET_SIZE(k, eigcut_row, ev, co, &rhs);
}

// ------------------------------------------------------------------------------------------
// Staging.  The plain assembly stages 64 entries x one row of 20 in LDS (15 KB).  64 entries x five rows would be 51 KB of values
// plus 26 KB of indices, beyond the 64 KB a workgroup may declare: a workgroup serves MULTI_TILE = 32 entries, lanes 0 .. 31 one
// each (25.6 + 12.8 KB); lanes 32 .. 63 hold no entry and help with the copy-out.  A head of 16384 entries is then 512 workgroups.
#define MULTI_TILE 32
#define MULTI_MAX_HEAD 16384
#define MULTI_MAX_BLOCKS (MULTI_MAX_HEAD / MULTI_TILE)
static_assert(MULTI_MAX_BLOCKS <= ROUND_AGG_WORDS, "a look-back word per workgroup");
static_assert(MULTI_TILE <= 64 && SDPCUT_MULTI_MAX_PER_SET <= SDPCUT_MAX_K, "one lane per entry; an entry has at most k violated eigenvalues");
static_assert(MULTI_TILE * SDPCUT_MULTI_MAX_PER_SET * SDPCUT_ROW_LD * 12 <= 64 * 1024, "staging must fit the LDS of a workgroup");

struct MultiCsrArgs {
    int64_t cap;               // head entries the block is laid out for
    int64_t limit;             // head entries that exist (<= cap)
    int64_t row_cap;           // rows numbered >= row_cap are dropped (min(row_quota, m * cap): the block holds row_cap rows)
    int32_t m;                 // rows an entry offers at most
    const int64_t *idx;        // [cap] global candidate ids of the head
    const double *score;       // [cap]
    int64_t idx_base, n_local;
    const int32_t *set5;       // [N][5]
    const int32_t *ks;         // [N]
    const double *vars;
    int32_t nv;
    int64_t L;
    // outputs: device view of the pinned host block (round_layout.h: csr_multi_layout)
    int64_t *o_hdr;            // [16]: 7 completion serial, 8 rows, 9 non-zeros, 10 look-back gave up, 11 a row was dropped (the host zeroes 8 .. 11)
    int64_t *o_idx;            // [cap]
    double *o_score, *o_lam;   // [cap]
    int32_t *o_ks, *o_sets, *o_nneg;   // [cap], [cap][5], [cap]
    int32_t *o_row_entry, *o_row_rank; // [row_cap]
    int32_t *o_indptr;         // [row_cap + 1]
    double *o_rhs, *o_row_lam; // [row_cap]
    int32_t *o_indices;        // [row_cap * ld]
    double *o_values;          // [row_cap * ld]
    int64_t serial;
    uint32_t *done_ticket;
    uint64_t *agg;             // [gridDim.x] look-back words
    int inject;                // SDPCUT_OPT_INJECT_GIVEUP: the look-back gives up unasked (rows_dev.h); 0 outside tests
};

__global__ __launch_bounds__(64) void multi_csr_kernel(MultiCsrArgs R)
{
    __shared__ double s_val[MULTI_TILE * SDPCUT_MULTI_MAX_PER_SET * SDPCUT_ROW_LD];
    __shared__ int32_t s_ind[MULTI_TILE * SDPCUT_MULTI_MAX_PER_SET * SDPCUT_ROW_LD];
    const int lane = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * MULTI_TILE;
    const int64_t i = first + lane;
    int64_t limit = R.limit;
    if (limit > R.cap) limit = R.cap;
    const bool live = lane < MULTI_TILE && i < limit;
    MultiEig E;
    int64_t cl[SDPCUT_ROW_LD];
#pragma unroll
    for (int m = 0; m < SDPCUT_ROW_LD; ++m) cl[m] = 0;
    E.n_neg = 0;
    E.lam_min = __builtin_nan("");
    int k = 0;
    if (live) {
        const int64_t gid = R.idx[i];
        R.o_idx[i] = gid;
        R.o_score[i] = R.score[i];
        const int64_t c = gid - R.idx_base;
        int32_t s5[5] = {-1, -1, -1, -1, -1};
        if (c >= 0 && c < R.n_local) {
            k = R.ks[c];
            const int32_t *sp = R.set5 + c * 5;
#pragma unroll
            for (int a = 0; a < 5; ++a) s5[a] = sp[a];
            multi_decompose_k(k, sp, R.vars, R.nv, R.L, E, cl);
        }
        R.o_lam[i] = E.lam_min;
        R.o_ks[i] = k;
        R.o_nneg[i] = E.n_neg;
#pragma unroll
        for (int a = 0; a < 5; ++a) R.o_sets[i * 5 + a] = s5[a];
    }
    // what the entry offers: its violated eigenpairs, at most m (they are the first n_neg of the ascending order)
    const int cnt = (live && k > 0) ? (E.n_neg < R.m ? E.n_neg : R.m) : 0;
    const int len = k * (k + 3) / 2;
    // position inside the workgroup (= one wave): rows and non-zeros in front of this lane's first row
    int incl_r = cnt, incl_z = cnt * len;
    for (int off = 1; off < 64; off <<= 1) {
        const int orr = __shfl_up(incl_r, off), oz = __shfl_up(incl_z, off);
        if (lane >= off) { incl_r += orr; incl_z += oz; }
    }
    const int my_row = incl_r - cnt, my_off = incl_z - cnt * len;
    const int wg_rows = __shfl(incl_r, 63), wg_nnz = __shfl(incl_z, 63);
    // publish this workgroup's aggregate (BEFORE the quota: a workgroup behind the quota must see it passed), then sum those in front
    int64_t pre_rows, pre_nnz;
    const int gave_up = csr_lookback(R.agg, (uint32_t)R.serial, wg_rows, wg_nnz, pre_rows, pre_nnz, R.inject);
    if (gave_up && lane == 0) R.o_hdr[10] = 1;      // the block is void; the host launches the assembly once more
    // The rows, now that their global numbers are known.  Row g of the round is kept iff g < row_cap; the row numbered row_cap
    // itself -- the first one dropped -- says where the block ends.  With a give-up the numbers are wrong but stay inside the
    // block (g < row_cap is still checked) and the host discards everything.
    int kept = 0;
    for (int r = 0; r < SDPCUT_MULTI_MAX_PER_SET; ++r) {
        if (r < cnt) {
            const int64_t g = pre_rows + my_row + r;
            const int lo = my_off + r * len;
            if (g < R.row_cap) {
                double ev[MULTI_DMAX], co[SDPCUT_ROW_LD], rhs = 0.0;
#pragma unroll
                for (int m = 0; m < SDPCUT_ROW_LD; ++m) co[m] = 0.0;
                const double lam_r = multi_pick(E, r, ev);
                multi_row_k(k, ev, co, rhs);
                R.o_row_entry[g] = (int32_t)i;
                R.o_row_rank[g] = r;
                R.o_row_lam[g] = lam_r;
                R.o_indptr[g] = (int32_t)(pre_nnz + lo);
                R.o_rhs[g] = rhs;
#pragma unroll
                for (int m = 0; m < SDPCUT_ROW_LD; ++m)
                    if (m < len) { s_val[lo + m] = co[m]; s_ind[lo + m] = (int32_t)cl[m]; }
                ++kept;
            } else if (g == R.row_cap && !gave_up) {
                R.o_indptr[g] = (int32_t)(pre_nnz + lo);
                R.o_hdr[8] = g;
                R.o_hdr[9] = pre_nnz + lo;
                R.o_hdr[11] = 1;
            }
        }
    }
    // kept rows are a prefix of the workgroup's rows: their non-zeros are a prefix of its staging area
    int kept_nnz = kept * len;
    for (int off = 32; off > 0; off >>= 1) kept_nnz += __shfl_xor(kept_nnz, off);
    wave_lds_sync();
    for (int w = lane; w < kept_nnz; w += 64) {      // contiguous, coalesced stores over PCIe
        R.o_values[pre_nnz + w] = s_val[w];
        R.o_indices[pre_nnz + w] = s_ind[w];
    }
    if (blockIdx.x == gridDim.x - 1 && lane == 0 && !gave_up && pre_rows + wg_rows <= R.row_cap) {      // nothing was dropped
        R.o_indptr[pre_rows + wg_rows] = (int32_t)(pre_nnz + wg_nnz);
        R.o_hdr[8] = pre_rows + wg_rows;
        R.o_hdr[9] = pre_nnz + wg_nnz;
    }
    publish_round_done(R.done_ticket, R.o_hdr + 7, R.serial);
}

// ------------------------------------------------------------------------------------------
// Rows of an explicit id list (local ids, validated by the host), one lane per entry: entry i writes its offered rows into the
// padded slots i * m + r of lam / coef / rhs and their number into n_off[i]; the host compacts.  cols / ks per entry as cut_rows_kernel.
__global__ __launch_bounds__(64) void cut_rows_all_kernel(int64_t count, int32_t m, const int64_t *idx, int64_t n_local,
                                                          const int32_t *set5, const int32_t *ks, const double *vars, int32_t nv,
                                                          int64_t L, int32_t *n_off, double *lam, double *coef, double *rhs,
                                                          int64_t *cols, int32_t *ks_out)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const int64_t c = idx[i];
    int64_t cl[SDPCUT_ROW_LD];
#pragma unroll
    for (int mm = 0; mm < SDPCUT_ROW_LD; ++mm) cl[mm] = -1;
    if (c < 0 || c >= n_local) {      // (the host refuses such a list; nothing is read through a bad id)
        n_off[i] = 0;
        ks_out[i] = 0;
#pragma unroll
        for (int mm = 0; mm < SDPCUT_ROW_LD; ++mm) cols[i * SDPCUT_ROW_LD + mm] = -1;
        return;
    }
    const int k = ks[c];
    MultiEig E;
    multi_decompose_k(k, set5 + c * 5, vars, nv, L, E, cl);
    const int cnt = E.n_neg < m ? E.n_neg : m;
    n_off[i] = cnt;
    ks_out[i] = k;
#pragma unroll
    for (int mm = 0; mm < SDPCUT_ROW_LD; ++mm) cols[i * SDPCUT_ROW_LD + mm] = cl[mm];
    for (int r = 0; r < SDPCUT_MULTI_MAX_PER_SET; ++r) {
        if (r < cnt) {
            double ev[MULTI_DMAX], co[SDPCUT_ROW_LD], rh = 0.0;
#pragma unroll
            for (int mm = 0; mm < SDPCUT_ROW_LD; ++mm) co[mm] = 0.0;
            const double lam_r = multi_pick(E, r, ev);
            multi_row_k(k, ev, co, rh);
            const int64_t slot = i * m + r;
            lam[slot] = lam_r;
            rhs[slot] = rh;
#pragma unroll
            for (int mm = 0; mm < SDPCUT_ROW_LD; ++mm) coef[slot * SDPCUT_ROW_LD + mm] = co[mm];
        }
    }
}

// ------------------------------------------------------------------------------------------
// what the multi-cut calls keep on the handle
struct MultiWs {
    DevBuf<int64_t> ids;             // [cap] the ranked head (sdpcut_rank_device); grows together with score
    DevBuf<double> score;
    // max_per_set = 1 forwards to the plain round, whose block has no room for the per-row extras: they live here
    std::vector<int32_t> h_nneg, h_rank;
    std::vector<double> h_rlam;
};

void free_multi_ws(sdpcut_ctx *h)
{
    delete (MultiWs *)h->multi;
    h->multi = nullptr;
}

static int multi_ensure(sdpcut_ctx *h, int64_t cap, MultiWs **out)
{
    MultiWs *w = (MultiWs *)h->multi;
    if (!w) {
        w = new (std::nothrow) MultiWs();
        if (!w) return sdpcut_fail(h, SDPCUT_ENOMEM, "out of host memory");
        h->multi = w;
    }
    int rc;
    if ((rc = grow(h, w->ids, (size_t)(cap < 0 ? 0 : cap))) || (rc = grow(h, w->score, (size_t)(cap < 0 ? 0 : cap)))) return rc;
    *out = w;
    return 0;
}

static int launch_multi_csr(sdpcut_ctx *h, MultiWs *w, int64_t cap, int64_t limit, int64_t row_cap, int32_t m, int ld, void *block,
                            int64_t serial)
{
    const int grid = (int)((cap + MULTI_TILE - 1) / MULTI_TILE);
    if (grid < 1 || grid > MULTI_MAX_BLOCKS) return sdpcut_fail(h, SDPCUT_EINVAL, "round_csr_multi: head too long");
    const int rc = ensure_round_sync(h);
    if (rc) return rc;
    MultiCsrArgs R;
    R.cap = cap; R.limit = limit; R.row_cap = row_cap; R.m = m; R.idx = w->ids.get(); R.score = w->score.get(); R.idx_base = h->base;
    R.n_local = h->N; R.set5 = h->d_set_orig.get(); R.ks = h->d_k.get(); R.vars = h->d_vars.get(); R.nv = h->nb_vars; R.L = h->L;
    const CsrMultiLayout y = csr_multi_layout(cap, row_cap, ld);
    char *b = (char *)block;
    R.o_hdr = (int64_t *)b;
    R.o_idx = (int64_t *)(b + y.idx); R.o_score = (double *)(b + y.score); R.o_lam = (double *)(b + y.lam);
    R.o_ks = (int32_t *)(b + y.ks); R.o_sets = (int32_t *)(b + y.sets); R.o_nneg = (int32_t *)(b + y.n_neg);
    R.o_row_entry = (int32_t *)(b + y.row_entry); R.o_row_rank = (int32_t *)(b + y.row_rank); R.o_indptr = (int32_t *)(b + y.indptr);
    R.o_rhs = (double *)(b + y.rhs); R.o_row_lam = (double *)(b + y.row_lam); R.o_indices = (int32_t *)(b + y.indices);
    R.o_values = (double *)(b + y.values);
    R.serial = serial; R.done_ticket = h->d_done_ticket.get(); R.agg = round_agg_words(h);
    R.inject = inject_take(h, 2, grid > 1);
    hipLaunchKernelGGL(multi_csr_kernel, dim3(grid), dim3(64), 0, h->stream, R);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// max_per_set = 1: the plain round, then the quota and the per-row extras on the host
static int multi_forward_one(sdpcut_ctx *h, const double *vars_values, int strat, int64_t sel_size, int64_t row_quota,
                             sdpcut_round_multi_t *out)
{
    int rc = sdpcut_round_csr(h, vars_values, strat, sel_size, &out->csr);
    if (rc) { std::memset(out, 0, sizeof(*out)); return rc; }
    sdpcut_round_csr_t &o = out->csr;
    out->row_cap = row_quota < o.cap ? row_quota : o.cap;
    if (o.cap == 0 || !o.idx) return SDPCUT_OK;
    MultiWs *w = nullptr;
    rc = multi_ensure(h, 0, &w);
    if (rc) return rc;
    if (o.n_rows > row_quota) {
        out->quota_hit = 1;
        o.n_rows = row_quota;
        o.nnz = o.indptr[row_quota];
    }
    w->h_nneg.assign((size_t)(o.n_out > 0 ? o.n_out : 1), 0);
    w->h_rank.assign((size_t)(o.n_rows > 0 ? o.n_rows : 1), 0);
    w->h_rlam.assign((size_t)(o.n_rows > 0 ? o.n_rows : 1), 0.0);
    for (int64_t i = 0; i < o.n_out; ++i) w->h_nneg[(size_t)i] = o.lam_min[i] < SDPCUT_NEG_EIGVAL ? 1 : 0;
    for (int64_t r = 0; r < o.n_rows; ++r) w->h_rlam[(size_t)r] = o.lam_min[o.row_entry[r]];
    out->n_neg = w->h_nneg.data();
    out->row_rank = w->h_rank.data();
    out->row_lam = w->h_rlam.data();
    out->n_used = o.n_rows > 0 ? 1 + (int64_t)o.row_entry[o.n_rows - 1] : 0;
    return SDPCUT_OK;
}

extern "C" {

int sdpcut_round_csr_multi(sdpcut_handle h, const double *vars_values, int strat, int64_t sel_size, int32_t max_per_set,
                           int64_t row_quota, sdpcut_round_multi_t *out)
{
    if (!h) return SDPCUT_EINVAL;
    if (!out) return sdpcut_fail(h, SDPCUT_EINVAL, "out is NULL");
    std::memset(out, 0, sizeof(*out));
    int rc;
    if (max_per_set < 1 || max_per_set > SDPCUT_MULTI_MAX_PER_SET)
        return sdpcut_fail(h, SDPCUT_EINVAL, "max_per_set must lie in 1 .. SDPCUT_MULTI_MAX_PER_SET");
    if (row_quota < 1) return sdpcut_fail(h, SDPCUT_EINVAL, "row_quota must be >= 1");
    const uint32_t measure = strat_view(h, strat);      // strategies 3 and 6 rank through a view (common.h: MeasureAsObj)
    if (!measure && (rc = check_round_strategy(h, strat))) return rc;
    if (sel_size < 0) return sdpcut_fail(h, SDPCUT_EINVAL, "bad round_csr_multi arguments");
    if (h->nb_vars == 0 || !h->d_eig.get() || !(h->have_point || vars_values))
        return sdpcut_fail(h, SDPCUT_ESTATE, "set_instance, set_candidates and a point first");
    SDPCUT_NO_PENDING(h);
    if (max_per_set == 1) return multi_forward_one(h, vars_values, strat, sel_size, row_quota, out);
    if (vars_values && (rc = sdpcut_set_point(h, vars_values))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const int64_t cap = sel_size < h->N ? sel_size : h->N;
    if (cap > MULTI_MAX_HEAD) return sdpcut_fail(h, SDPCUT_EINVAL, "round_csr_multi: head too long");
    // the head: the strategy's ranking by the existing ranking call, as the plain round's general path ranks it
    if (!measure && cap > 0 && exact_head_applies(h, strat) && exact_first_band(h, cap) > TK_LDSK)
        return sdpcut_fail(h, SDPCUT_EINVAL, "SDPCUT_OPT_EXACT_HEAD: the head plus its band (min(N, sel_size + max(256, sel_size / 8))) must not exceed 8192 entries");
    const uint32_t need = measure ? measure : strat_need(strat);
    if ((rc = obj_complete(h))) return rc;      // a measure a skipped round left partial: whole before this round counts by it
    if ((h->scored & need) != need && (rc = sdpcut_score(h, need & ~h->scored))) return rc;
    sdpcut_round_csr_t &o = out->csr;
    o.row_ld = h->row_len_max;
    if (cap == 0) return sdpcut_rank(h, strat, sel_size, 0, nullptr, nullptr, &o.n_total, &o.new_strat, o.counters);
    MultiWs *w = nullptr;
    rc = multi_ensure(h, cap, &w);
    if (rc) return rc;
    int64_t P = 0;
    rc = sdpcut_rank_device(h, strat, sel_size, cap, w->ids.get(), w->score.get(), &P, &o.n_total, &o.new_strat, o.counters);
    if (rc) return rc;
    if (P > cap) P = cap;
    const int64_t all_rows = (int64_t)max_per_set * cap;
    const int64_t row_cap = row_quota < all_rows ? row_quota : all_rows;
    const int32_t ld = h->row_len_max;
    const CsrMultiLayout y = csr_multi_layout(cap, row_cap, ld);
    rc = ensure_pinned(h, y.bytes);
    if (rc) return rc;
    const int64_t *hdr = (const int64_t *)h->pinned.get();
    rc = csr_assemble_wait(h, 11, 2, true, "round_csr_multi", [&](int64_t serial) {
        return launch_multi_csr(h, w, cap, P, row_cap, max_per_set, ld, h->pinned.dev(), serial);
    });
    if (rc) return rc;
    ++h->stat_rounds;
    const char *b = (const char *)h->pinned.get();
    o.cap = cap;
    o.n_out = P;
    o.idx = (const int64_t *)(b + y.idx);
    o.score = (const double *)(b + y.score);
    o.lam_min = (const double *)(b + y.lam);
    o.ks = (const int32_t *)(b + y.ks);
    o.set_inds = (const int32_t *)(b + y.sets);
    o.n_rows = hdr[8];
    o.nnz = hdr[9];
    o.row_entry = (const int32_t *)(b + y.row_entry);
    o.indptr = (const int32_t *)(b + y.indptr);
    o.indices = (const int32_t *)(b + y.indices);
    o.values = (const double *)(b + y.values);
    o.rhs = (const double *)(b + y.rhs);
    out->row_cap = row_cap;
    out->quota_hit = hdr[11] ? 1 : 0;
    out->n_neg = (const int32_t *)(b + y.n_neg);
    out->row_lam = (const double *)(b + y.row_lam);
    out->row_rank = (const int32_t *)(b + y.row_rank);
    out->n_used = o.n_rows > 0 ? 1 + (int64_t)o.row_entry[o.n_rows - 1] : 0;
    return SDPCUT_OK;
}

int sdpcut_cut_rows_all(sdpcut_handle h, int64_t count, const int64_t *idx, int32_t max_per_set, int64_t *row_ptr, double *row_lam,
                        double *coef, double *rhs, int64_t *cols, int32_t *ks)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (max_per_set < 1 || max_per_set > SDPCUT_MULTI_MAX_PER_SET)
        return sdpcut_fail(h, SDPCUT_EINVAL, "max_per_set must lie in 1 .. SDPCUT_MULTI_MAX_PER_SET");
    if (!h->have_point || !h->d_set_orig.get()) return sdpcut_fail(h, SDPCUT_ESTATE, "set_candidates and set_point first");
    if (count < 0 || !row_ptr || (count > 0 && (!idx || !row_lam || !coef || !rhs || !cols || !ks)))
        return sdpcut_fail(h, SDPCUT_EINVAL, "bad cut_rows_all arguments");
    row_ptr[0] = 0;
    if (count == 0) return SDPCUT_OK;
    for (int64_t i = 0; i < count; ++i)
        if (idx[i] < 0 || idx[i] >= h->N) return sdpcut_fail(h, SDPCUT_EINVAL, "candidate index out of range");
    const size_t c = (size_t)count, LD = SDPCUT_ROW_LD;
    if (max_per_set == 1) {
        // the rows sdpcut_cut_rows gives (same kernel, same eigenvector route), kept where lam_min is violated
        int rc = sdpcut_cut_rows(h, count, idx, row_lam, coef, rhs, cols, ks);
        if (rc) return rc;
        int64_t n = 0;
        for (size_t i = 0; i < c; ++i) {
            if (row_lam[i] < SDPCUT_NEG_EIGVAL) {
                if ((size_t)n != i) {
                    row_lam[n] = row_lam[i];
                    rhs[n] = rhs[i];
                    std::memmove(coef + (size_t)n * LD, coef + i * LD, LD * 8);
                }
                ++n;
            }
            row_ptr[i + 1] = n;
        }
        return SDPCUT_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t m = (size_t)max_per_set;
    // staging layout: idx | lam [c m] | rhs [c m] | coef [c m][LD] | cols [c][LD] | ks | n_off
    const size_t bytes = c * 8 + c * m * 8 * (2 + LD) + c * 8 * LD + c * 8;
    int rc = ensure_stage(h, bytes);
    if (rc) return rc;
    char *p = (char *)h->d_stage.get();
    int64_t *d_idx = (int64_t *)p; p += c * 8;
    double *d_lam = (double *)p; p += c * m * 8;
    double *d_rhs = (double *)p; p += c * m * 8;
    double *d_coef = (double *)p; p += c * m * 8 * LD;
    int64_t *d_cols = (int64_t *)p; p += c * 8 * LD;
    int32_t *d_ks = (int32_t *)p; p += c * 4;
    int32_t *d_off = (int32_t *)p;
    std::vector<int32_t> n_off;
    try {
        n_off.resize(c);
    } catch (const std::bad_alloc &) {
        return sdpcut_fail(h, SDPCUT_ENOMEM, "out of host memory");
    }
    HIP_TRY(h, hipMemcpyAsync(d_idx, idx, c * 8, hipMemcpyHostToDevice, h->stream));
    // slots an entry does not fill are never read back as rows, but they travel: keep them defined
    HIP_TRY(h, hipMemsetAsync(d_lam, 0, c * m * 8 * (2 + LD), h->stream));
    const int grid = (int)((count + 63) / 64);
    hipLaunchKernelGGL(cut_rows_all_kernel, dim3(grid), dim3(64), 0, h->stream, count, max_per_set, d_idx, h->N, h->d_set_orig.get(), h->d_k.get(),
                       h->d_vars.get(), h->nb_vars, h->L, d_off, d_lam, d_coef, d_rhs, d_cols, d_ks);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(row_lam, d_lam, c * m * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(rhs, d_rhs, c * m * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(coef, d_coef, c * m * 8 * LD, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(cols, d_cols, c * 8 * LD, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(ks, d_ks, c * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(n_off.data(), d_off, c * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    // compact the padded slots i * m + r to rows, in place (a row never moves backwards)
    int64_t n = 0;
    for (size_t i = 0; i < c; ++i) {
        for (int32_t r = 0; r < n_off[i]; ++r) {
            const size_t slot = i * m + (size_t)r;
            if ((size_t)n != slot) {
                row_lam[n] = row_lam[slot];
                rhs[n] = rhs[slot];
                std::memmove(coef + (size_t)n * LD, coef + slot * LD, LD * 8);
            }
            ++n;
        }
        row_ptr[i + 1] = n;
    }
    return SDPCUT_OK;
}

} // extern "C"
