// Staging round trips of the extern "C" surface (include/sdpcut.h): host arrays in, one kernel family, host arrays out --
// scores, rankings and their windows, cut rows, the batched eigen / network / triangle entries.
#include <cstring>

#include "common.h"
#include "topk_route.h"

int obj_complete(sdpcut_ctx *h)
{
    return h->obj_partial ? sdpcut_score(h, SDPCUT_NN) : 0;
}

extern "C" {

int sdpcut_score(sdpcut_handle h, uint32_t flags)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (!(flags & (SDPCUT_EIG | SDPCUT_NN | SDPCUT_SDP | SDPCUT_EFF)) || (flags & ~(uint32_t)(SDPCUT_EIG | SDPCUT_NN | SDPCUT_SDP | SDPCUT_EFF)))
        return sdpcut_fail(h, SDPCUT_EINVAL, "flags must be a combination of SDPCUT_EIG, SDPCUT_NN, SDPCUT_SDP and SDPCUT_EFF");
    if ((flags & SDPCUT_EFF) && !(h->scored & SDPCUT_EIG)) flags |= SDPCUT_EIG;      // the efficacy is that of the row of the lambda_min the handle holds
    if (!h->have_point) return sdpcut_fail(h, SDPCUT_ESTATE, "set_point first");
    if (!h->d_eig.get()) return sdpcut_fail(h, SDPCUT_ESTATE, "set_candidates first");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    if (flags & (SDPCUT_EIG | SDPCUT_NN)) {
        rc = launch_score(h, flags & (SDPCUT_EIG | SDPCUT_NN));   // with SDPCUT_OPT_TIMING the dispatches carry ev[0] / ev[1]
        if (rc) return rc;
    }
    if (flags & SDPCUT_SDP) {      // its own kernels and arrays (exact_sdp.hip): no network needed, d_eig / d_obj untouched
        rc = launch_exact_sdp(h);
        if (rc) return rc;
    }
    if (flags & SDPCUT_EFF) {      // after SDPCUT_EIG on the stream; its own kernel and arrays (efficacy.hip), no network needed
        rc = launch_efficacy(h);
        if (rc) return rc;
    }
    h->scored |= flags;
    return SDPCUT_OK;
}

int sdpcut_get_scores(sdpcut_handle h, double *eigmin, double *obj_improve)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    if (obj_improve && (rc = obj_complete(h))) return rc;
    if (eigmin) {
        if (!(h->scored & SDPCUT_EIG)) return sdpcut_fail(h, SDPCUT_ESTATE, "eigenvalues not scored");
        HIP_TRY(h, hipMemcpyAsync(eigmin, h->d_eig.get(), h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    if (obj_improve) {
        if (!(h->scored & SDPCUT_NN)) return sdpcut_fail(h, SDPCUT_ESTATE, "optimality measure not scored");
        HIP_TRY(h, hipMemcpyAsync(obj_improve, h->d_obj, h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

static int check_rank_args(sdpcut_ctx *h, int strat)
{
    int rc;
    if (strat != SDPCUT_PART_STRONG && (rc = check_round_strategy(h, strat))) return rc;
    const uint32_t need = strat_need(strat);
    if ((rc = obj_complete(h))) return rc;      // (a feasibility ranking too: its nb_positive reads the measure)
    if ((h->scored & need) != need) return sdpcut_fail(h, SDPCUT_ESTATE, "sdpcut_score with the needed flags first");
    return 0;
}
int sdpcut_rank_device(sdpcut_handle h, int strat, int64_t sel_size, int64_t max_out, void *d_idx_out,
                       void *d_score_out, int64_t *n_written, int64_t *n_total, int32_t *new_strat,
                       int64_t *counters)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (const uint32_t measure = strat_view(h, strat)) {      // strategy 2 on the exact measure (3) / on the efficacy score (6)
        if (!(h->scored & measure)) return sdpcut_fail(h, SDPCUT_ESTATE, "sdpcut_score with the needed flags first");
        MeasureAsObj view(h, measure);
        const int rc3 = sdpcut_rank_device(h, SDPCUT_STRAT_OPT, sel_size, max_out, d_idx_out, d_score_out, n_written, n_total, new_strat, counters);
        if (!rc3 && new_strat) *new_strat = view_strat(measure);
        return rc3;
    }
    int rc = check_rank_args(h, strat);
    if (rc) return rc;
    if (max_out < 0 || (max_out > 0 && (!d_idx_out || !d_score_out))) return sdpcut_fail(h, SDPCUT_EINVAL, "bad output");
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->timing > 1) HIP_TRY(h, hipEventRecord(h->ev[2], h->stream));
    h->stat_exact_last = 0;
    {
        // SDPCUT_OPT_EXACT_HEAD: heads within the limit (strategy 4: a head of the scan's own length at most, whose regime the
        // device resolves) are ordered by reference-order obj_improve; whatever it cannot serve ranks as with the option off
        const int64_t cap = max_out < h->N ? max_out : h->N, sel = sel_size < h->N ? sel_size : h->N;
        if (cap >= 1 && exact_head_applies(h, strat) && exact_first_band(h, cap) <= TK_LDSK && (strat != SDPCUT_STRAT_COMB || cap <= sel)) {
            int64_t band = exact_first_band(h, cap);
            for (int attempt = 0; attempt < 2; ++attempt) {
                const int64_t *d_c4 = nullptr;
                int64_t c4[7] = {0, 0, 0, 0, 0, 0, 0};
                rc = exact_head_enqueue(h, strat, sel_size, cap, band, (int64_t *)d_idx_out, (double *)d_score_out, &d_c4);
                if (rc) return rc;
                HIP_TRY(h, hipMemcpyAsync(c4, d_c4, 7 * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
                HIP_TRY(h, sdpcut_sync(h));
                const int v = exact_head_verdict(h, c4, band);
                if (v == 0 && rank_fast_finish(h, strat, sel_size, cap, c4, n_written, n_total, new_strat, counters)) {
                    h->stat_exact_last = 1;
                    if (h->timing > 1) HIP_TRY(h, hipEventRecord(h->ev[3], h->stream));
                    return SDPCUT_OK;
                }
                if (v != 1 || attempt == 1) break;
                ++h->stat_exact_retries;
                band = exact_widest_band(h);
            }
            ++h->stat_exact_gave_up;
        }
    }
    rc = rank_on_device(h, strat, sel_size, max_out, (int64_t *)d_idx_out, (double *)d_score_out, n_written, n_total,
                        new_strat, counters);
    if (rc) return rc;
    if (h->timing > 1) HIP_TRY(h, hipEventRecord(h->ev[3], h->stream));
    return SDPCUT_OK;
}

int sdpcut_rank(sdpcut_handle h, int strat, int64_t sel_size, int64_t max_out, int64_t *idx_out, double *score_out,
                int64_t *n_total, int32_t *new_strat, int64_t *counters)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (max_out < 0 || (max_out > 0 && (!idx_out || !score_out))) return sdpcut_fail(h, SDPCUT_EINVAL, "bad output");
    HIP_TRY(h, hipSetDevice(h->device));
    int64_t cap = max_out < h->N ? max_out : h->N;
    int rc = ensure_stage(h, (size_t)(cap < 1 ? 1 : cap) * 16);
    if (rc) return rc;
    int64_t *d_idx = (int64_t *)h->d_stage.get();
    double *d_sc = (double *)((char *)h->d_stage.get() + (size_t)(cap < 1 ? 1 : cap) * 8);
    int64_t w = 0;
    rc = sdpcut_rank_device(h, strat, sel_size, cap, d_idx, d_sc, &w, n_total, new_strat, counters);
    if (rc) return rc;
    if (w > 0) {
        HIP_TRY(h, hipMemcpyAsync(idx_out, d_idx, w * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(score_out, d_sc, w * 8, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

int sdpcut_rank_fetch(sdpcut_handle h, int64_t offset, int64_t count, int64_t *idx_out, double *score_out)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (h->last_total < 0) return sdpcut_fail(h, SDPCUT_ESTATE, "no ranking available: call sdpcut_rank first");
    if (offset < 0 || count < 0 || offset + count > h->last_total || (count > 0 && (!idx_out || !score_out)))
        return sdpcut_fail(h, SDPCUT_EINVAL, "window outside the last ranking");
    if (count == 0) return SDPCUT_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = ensure_stage(h, (size_t)count * 16);
    if (rc) return rc;
    int64_t *d_idx = (int64_t *)h->d_stage.get();
    double *d_sc = (double *)((char *)h->d_stage.get() + (size_t)count * 8);
    rc = rank_fetch_on_device(h, offset, count, d_idx, d_sc);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(idx_out, d_idx, count * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(score_out, d_sc, count * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

int sdpcut_merge_topk_device(sdpcut_handle h, int64_t count, const void *d_scores, const void *d_secondary,
                             const void *d_ids, int64_t max_out, void *d_score_out, void *d_id_out)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (count < 0 || max_out < 0 || (count > 0 && max_out > 0 && (!d_scores || !d_ids || !d_score_out || !d_id_out)))
        return sdpcut_fail(h, SDPCUT_EINVAL, "bad merge arguments");
    if (count > 0x7fffffffLL) return sdpcut_fail(h, SDPCUT_EINVAL, "merge too large");
    HIP_TRY(h, hipSetDevice(h->device));
    return merge_topk_on_device(h, count, (const double *)d_scores, (const double *)d_secondary,
                                (const int64_t *)d_ids, max_out, (double *)d_score_out, (int64_t *)d_id_out);
}

int sdpcut_gather_scores_device(sdpcut_handle h, int64_t count, const void *d_ids, void *d_eig_out, void *d_obj_out)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (count < 0 || (count > 0 && !d_ids)) return sdpcut_fail(h, SDPCUT_EINVAL, "bad gather arguments");
    int rc;
    if (d_obj_out && (rc = obj_complete(h))) return rc;
    if ((d_eig_out && !(h->scored & SDPCUT_EIG)) || (d_obj_out && !(h->scored & SDPCUT_NN)))
        return sdpcut_fail(h, SDPCUT_ESTATE, "sdpcut_score with the needed flags first");
    HIP_TRY(h, hipSetDevice(h->device));
    return gather_scores_on_device(h, count, (const int64_t *)d_ids, (double *)d_eig_out, (double *)d_obj_out);
}

int sdpcut_cut_rows(sdpcut_handle h, int64_t count, const int64_t *idx, double *lam_min, double *coef, double *rhs,
                    int64_t *cols, int32_t *ks)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (!h->have_point || !h->d_set_orig.get()) return sdpcut_fail(h, SDPCUT_ESTATE, "set_candidates and set_point first");
    if (count < 0 || (count > 0 && (!idx || !lam_min || !coef || !rhs || !cols || !ks)))
        return sdpcut_fail(h, SDPCUT_EINVAL, "bad cut_rows arguments");
    if (count == 0) return SDPCUT_OK;
    for (int64_t i = 0; i < count; ++i)
        if (idx[i] < 0 || idx[i] >= h->N) return sdpcut_fail(h, SDPCUT_EINVAL, "candidate index out of range");
    HIP_TRY(h, hipSetDevice(h->device));
    // staging layout: idx | lam | rhs | coef | cols | ks
    const size_t c = (size_t)count;
    const size_t bytes = c * 8 * (3 + 2 * SDPCUT_ROW_LD) + c * 4;
    int rc = ensure_stage(h, bytes);
    if (rc) return rc;
    char *p = (char *)h->d_stage.get();
    int64_t *d_idx = (int64_t *)p; p += c * 8;
    double *d_lam = (double *)p; p += c * 8;
    double *d_rhs = (double *)p; p += c * 8;
    double *d_coef = (double *)p; p += c * 8 * SDPCUT_ROW_LD;
    int64_t *d_cols = (int64_t *)p; p += c * 8 * SDPCUT_ROW_LD;
    int32_t *d_ks = (int32_t *)p;
    HIP_TRY(h, hipMemcpyAsync(d_idx, idx, c * 8, hipMemcpyHostToDevice, h->stream));
    rc = launch_cut_rows(h, count, nullptr, d_idx, 0, d_lam, d_coef, SDPCUT_ROW_LD, d_rhs, d_cols, d_ks);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(lam_min, d_lam, c * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(rhs, d_rhs, c * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(coef, d_coef, c * 8 * SDPCUT_ROW_LD, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(cols, d_cols, c * 8 * SDPCUT_ROW_LD, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(ks, d_ks, c * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

int sdpcut_eig_batch(sdpcut_handle h, int k, int64_t count, const double *x_rho, const double *X_rho,
                     double *eigvals, double *evecs)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (k < 2 || k > SDPCUT_MAX_K) return sdpcut_fail(h, SDPCUT_EINVAL, "k must be 2..5");
    if (count < 0 || (count > 0 && (!x_rho || !X_rho || !eigvals))) return sdpcut_fail(h, SDPCUT_EINVAL, "bad eig_batch arguments");
    if (count == 0) return SDPCUT_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t c = (size_t)count, m = (size_t)k * (k + 1) / 2, D = (size_t)k + 1;
    const size_t bytes = c * 8 * (k + m + D + D * D);
    int rc = ensure_stage(h, bytes);
    if (rc) return rc;
    double *d_x = (double *)h->d_stage.get(), *d_X = d_x + c * k, *d_w = d_X + c * m, *d_v = d_w + c * D;
    HIP_TRY(h, hipMemcpyAsync(d_x, x_rho, c * k * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(d_X, X_rho, c * m * 8, hipMemcpyHostToDevice, h->stream));
    rc = launch_eig_batch(h, k, count, d_x, d_X, d_w, evecs ? d_v : nullptr);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(eigvals, d_w, c * D * 8, hipMemcpyDeviceToHost, h->stream));
    if (evecs) HIP_TRY(h, hipMemcpyAsync(evecs, d_v, c * D * D * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

int sdpcut_nn_batch(sdpcut_handle h, int k, int64_t count, const double *inputs, double *out)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (k < 2 || k > SDPCUT_MAX_K) return sdpcut_fail(h, SDPCUT_EINVAL, "k must be 2..5");
    if (!h->net[k].set) return sdpcut_fail(h, SDPCUT_ESTATE, "no network set for this candidate size");
    if (count < 0 || (count > 0 && (!inputs || !out))) return sdpcut_fail(h, SDPCUT_EINVAL, "bad nn_batch arguments");
    if (count == 0) return SDPCUT_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t c = (size_t)count, d = (size_t)k * (k + 3) / 2;
    int rc = ensure_stage(h, c * 8 * (d + 1));
    if (rc) return rc;
    double *d_in = (double *)h->d_stage.get(), *d_out = d_in + c * d;
    HIP_TRY(h, hipMemcpyAsync(d_in, inputs, c * d * 8, hipMemcpyHostToDevice, h->stream));
    rc = launch_nn_batch(h, k, count, d_in, d_out);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(out, d_out, c * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

int sdpcut_tri_preprocess(sdpcut_handle h, const uint8_t *adjacency, int64_t *n_triples)
{
    if (!h) return SDPCUT_EINVAL;
    if (h->nb_vars == 0) return sdpcut_fail(h, SDPCUT_ESTATE, "set_instance first");
    if (!adjacency) return sdpcut_fail(h, SDPCUT_EINVAL, "adjacency is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sdpcut_sync(h));
    return tri_preprocess(h, adjacency, n_triples);
}

int sdpcut_tri_get_triples(sdpcut_handle h, int32_t *triples_out, uint8_t *density_out)
{
    if (!h) return SDPCUT_EINVAL;
    if (h->n_tri > 0 && !triples_out) return sdpcut_fail(h, SDPCUT_EINVAL, "triples_out is NULL");
    if (h->n_tri > 0) std::memcpy(triples_out, h->tri_host.data(), (size_t)h->n_tri * 3 * sizeof(int32_t));
    if (density_out)
        for (int64_t t = 0; t < h->n_tri; ++t) density_out[t] = h->tri_dense_host[t] ? 3 : 2;
    return SDPCUT_OK;
}

int sdpcut_tri_separate(sdpcut_handle h, int64_t max_out, int64_t *entry_out, double *viol_out, int64_t *n_violated,
                        int64_t *n_written)
{
    if (!h) return SDPCUT_EINVAL;
    SDPCUT_NO_PENDING(h);
    if (!h->have_point) return sdpcut_fail(h, SDPCUT_ESTATE, "set_point first");
    if (max_out < 0 || (max_out > 0 && (!entry_out || !viol_out)) || !n_violated || !n_written)
        return sdpcut_fail(h, SDPCUT_EINVAL, "bad tri_separate arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    int64_t cap = max_out < 4 * h->n_tri ? max_out : 4 * h->n_tri;
    int rc = ensure_stage(h, (size_t)(cap < 1 ? 1 : cap) * 16);
    if (rc) return rc;
    int64_t *d_e = (int64_t *)h->d_stage.get();
    double *d_v = (double *)((char *)h->d_stage.get() + (size_t)(cap < 1 ? 1 : cap) * 8);
    int64_t w = 0;
    rc = tri_separate(h, cap, d_e, d_v, n_violated, &w);
    if (rc) return rc;
    if (w > 0) {
        HIP_TRY(h, hipMemcpyAsync(entry_out, d_e, w * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(viol_out, d_v, w * 8, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, sdpcut_sync(h));
    *n_written = w;
    return SDPCUT_OK;
}

} // extern "C"
