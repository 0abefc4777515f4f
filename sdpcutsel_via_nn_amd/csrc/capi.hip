// extern "C" surface of libsdpcut_hip.so (declared in include/sdpcut.h): the handle itself -- error text, create / destroy,
// options, statistics, stream, timing -- and its staging blocks.  The inputs are in inputs.hip, the staging round trips
// in batch.hip, the fused round in round.hip.
#include <cstring>
#include <mutex>
#include <new>

#include "common.h"

static std::string g_create_err;
static std::mutex g_mu;

int sdpcut_fail(sdpcut_ctx *h, int code, const std::string &msg)
{
    if (h) h->err = msg;
    else {
        std::lock_guard<std::mutex> lk(g_mu);
        g_create_err = msg;
    }
    return code;
}

int ensure_stage(sdpcut_ctx *h, size_t bytes) { return grow(h, h->d_stage, bytes); }

// Pinned host block the device can also write (kernel stores = the device-to-host transfer).
int ensure_pinned(sdpcut_ctx *h, size_t bytes)
{
    bool grew = false;
    const int rc = grow(h, h->pinned, bytes, &grew);
    if (rc) return rc;
    if (grew) std::memset(h->pinned.get(), 0, bytes < 64 ? bytes : 64);     // header incl. the completion word of wait_round_done
    return 0;
}

extern "C" {

int sdpcut_version(void) { return 200; }

const char *sdpcut_last_error(sdpcut_handle h)
{
    if (h) return h->err.c_str();
    std::lock_guard<std::mutex> lk(g_mu);
    return g_create_err.c_str();
}

int sdpcut_create(int device_id, sdpcut_handle *out)
{
    if (!out) return sdpcut_fail(nullptr, SDPCUT_EINVAL, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return sdpcut_fail(nullptr, SDPCUT_ENODEVICE,
                           "no HIP device visible: this library has no CPU fallback");
    if (device_id < 0 || device_id >= ndev) return sdpcut_fail(nullptr, SDPCUT_EINVAL, "device_id out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess)
        return sdpcut_fail(nullptr, SDPCUT_EHIP, "hipGetDeviceProperties failed");
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return sdpcut_fail(nullptr, SDPCUT_ENODEVICE,
                           std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    sdpcut_ctx *h = new (std::nothrow) sdpcut_ctx();
    if (!h) return sdpcut_fail(nullptr, SDPCUT_ENOMEM, "out of host memory");
    h->device = device_id;
    h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess ||
        h->d_counters.reset(8) != hipSuccess || h->d_stats.reset(8) != hipSuccess ||
        hipMemset(h->d_stats.get(), 0, 8 * sizeof(unsigned long long)) != hipSuccess) {
        delete h;
        return sdpcut_fail(nullptr, SDPCUT_EHIP, "stream / counter allocation failed");
    }
    h->stream = h->own_stream;
    for (int i = 0; i < 4; ++i) hipEventCreate(&h->ev[i]);
    *out = h;
    return SDPCUT_OK;
}

int sdpcut_destroy(sdpcut_handle h)
{
    if (!h) return SDPCUT_OK;
    hipSetDevice(h->device);
    sdpcut_sync(h);
    // the workspaces behind opaque members; everything else the handle owns frees itself with it
    free_diverse_ws(h);
    free_multi_ws(h);
    free_pool_ws(h);
    free_tri_points_ws(h);
    free_node_eval_ws(h);
    for (int i = 0; i < 4; ++i) if (h->ev[i]) hipEventDestroy(h->ev[i]);
    for (int i = 0; i < 3; ++i) {
        if (h->side_stream[i]) hipStreamDestroy(h->side_stream[i]);
        if (h->ev_join[i]) hipEventDestroy(h->ev_join[i]);
    }
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_switch) hipEventDestroy(h->ev_switch);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
    delete h;
    return SDPCUT_OK;
}

int sdpcut_set_option(sdpcut_handle h, int option, int64_t value)
{
    if (!h) return SDPCUT_EINVAL;
    switch (option) {
    case SDPCUT_OPT_KERNEL:
        if (value != SDPCUT_KERNEL_MFMA && value != SDPCUT_KERNEL_SIMPLE && value != SDPCUT_KERNEL_VALU)
            return sdpcut_fail(h, SDPCUT_EINVAL, "unknown kernel variant");
        if ((int)value != h->kernel_variant) {
            // the variants agree on the optimality measure to rounding, not to the bit: like the scores of a replaced network
            // (sdpcut_set_network) those of the old variant are not what the next call would compute -- it scores again
            SDPCUT_NO_PENDING(h);
            h->scored &= ~(uint32_t)SDPCUT_NN; h->obj_partial = false;
        }
        h->kernel_variant = (int)value;
        return SDPCUT_OK;
    case SDPCUT_OPT_FUSE_KEYS:
        h->fuse_keys = value != 0;
        return SDPCUT_OK;
    case SDPCUT_OPT_COOP_LAUNCH:
        h->coop_launch = value != 0;
        return SDPCUT_OK;
    case SDPCUT_OPT_FUSED_TAIL:
        h->fused_tail = value != 0;
        return SDPCUT_OK;
    case SDPCUT_OPT_AUTO_REGIME:
        h->auto_regime = value != 0;
        return SDPCUT_OK;
    case SDPCUT_OPT_EIG_KERNEL:
        h->eig_kernel = value != 0;
        return SDPCUT_OK;
    case SDPCUT_OPT_TIMING:
        h->timing = value <= 0 ? 0 : (value == 1 ? 1 : 2);
        return SDPCUT_OK;
    case SDPCUT_OPT_ONE_LAUNCH:
        h->one_launch = value != 0;
        return SDPCUT_OK;
    case SDPCUT_OPT_PREFILTER:
        h->prefilter = value != 0;
        return SDPCUT_OK;
    case SDPCUT_OPT_COUNT_RANK:
        h->count_rank = value != 0;
        return SDPCUT_OK;
    case SDPCUT_OPT_SKIP_NONVIOLATED:
        SDPCUT_NO_PENDING(h);
        if (value < 0 || value > 2) return sdpcut_fail(h, SDPCUT_EINVAL, "SDPCUT_OPT_SKIP_NONVIOLATED: 0 never, 1 long lists, 2 every list");
        h->skip_nonviolated = (int)value;
        return SDPCUT_OK;
    case SDPCUT_OPT_FP32_FILTER:
        SDPCUT_NO_PENDING(h);
        h->fp32_filter = value != 0;
        return SDPCUT_OK;
    case SDPCUT_OPT_EMIT_HEAD:
        SDPCUT_NO_PENDING(h);
        h->emit_head = value != 0;
        return SDPCUT_OK;
    case SDPCUT_OPT_EMIT_CAP:
        SDPCUT_NO_PENDING(h);
        if (value < 0) return sdpcut_fail(h, SDPCUT_EINVAL, "SDPCUT_OPT_EMIT_CAP: 0, or the capacity in entries");
        h->emit_cap_opt = value;
        return SDPCUT_OK;
    case SDPCUT_OPT_EXACT_HEAD:
        SDPCUT_NO_PENDING(h);
        if (value != 0) SDPCUT_NO_BOX(h, "SDPCUT_OPT_EXACT_HEAD");      // (the reference has no boxes: no reference-exact bits at a node)
        h->exact_head = value != 0;
        return SDPCUT_OK;
    case SDPCUT_OPT_EXACT_SDP:
        SDPCUT_NO_PENDING(h);
        h->exact_sdp = value != 0;
        return SDPCUT_OK;
    case SDPCUT_OPT_INJECT_GIVEUP: {
        SDPCUT_NO_PENDING(h);
        const int64_t site = value >> 16, first = (value >> 8) & 255, count = value & 255;
        if (value != 0 && (value < 0 || (site != 1 && site != 2) || count < 1))
            return sdpcut_fail(h, SDPCUT_EINVAL, "SDPCUT_OPT_INJECT_GIVEUP: 0, or SDPCUT_INJECT_GIVEUP(site 1..2, first 0..255, count 1..255)");
        h->inject_site = (int)site;
        h->inject_skip = (int)first;
        h->inject_count = (int)count;
        return SDPCUT_OK;
    }
    case SDPCUT_OPT_SIDE_STREAMS:
        if (value < 0 || value > 2) return sdpcut_fail(h, SDPCUT_EINVAL, "SDPCUT_OPT_SIDE_STREAMS: 0 off, 1 on, 2 measured");
        h->side_streams = (int)value;
        h->side_choice = -1;
        return SDPCUT_OK;
    case SDPCUT_OPT_STREAM_PRIORITY: {
        SDPCUT_NO_PENDING(h);
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, sdpcut_sync(h));
        int least = 0, greatest = 0;
        HIP_TRY(h, hipDeviceGetStreamPriorityRange(&least, &greatest));
        hipStream_t s = nullptr;
        // (0 = the priority hipStreamCreateWithFlags gives: normal, which lies between the two ends of the range)
        HIP_TRY(h, hipStreamCreateWithPriority(&s, hipStreamNonBlocking, value != 0 ? greatest : (0 < greatest ? greatest : (0 > least ? least : 0))));
        const bool on_own = h->stream == h->own_stream;
        if (h->own_stream) {
            HIP_TRY(h, hipStreamSynchronize(h->own_stream));
            (void)hipStreamDestroy(h->own_stream);
        }
        h->own_stream = s;
        if (on_own) h->stream = s;
        return SDPCUT_OK;
    }
    }
    return sdpcut_fail(h, SDPCUT_EINVAL, "unknown option");
}

int sdpcut_get_stat(sdpcut_handle h, int which, int64_t *value)
{
    if (!h || !value) return SDPCUT_EINVAL;
    switch (which) {
    case SDPCUT_STAT_ROUNDS: *value = h->stat_rounds; return SDPCUT_OK;
    case SDPCUT_STAT_SELECT_FALLBACKS: *value = h->stat_fallbacks; return SDPCUT_OK;
    // (a skipped round has scored the optimality measure -- of every candidate its ranking reads; the rest follows on demand)
    case SDPCUT_STAT_SCORED: *value = h->have_point ? (int64_t)(h->scored | (h->obj_partial ? (uint32_t)SDPCUT_NN : 0u)) : 0; return SDPCUT_OK;
    case SDPCUT_STAT_NN_COMPLETIONS: *value = h->stat_nn_completions; return SDPCUT_OK;
    case SDPCUT_STAT_NN_EVALUATED:
        if (h->nn_eval_mode == 2) {
            unsigned long long v = 0;
            HIP_TRY(h, hipSetDevice(h->device));
            HIP_TRY(h, hipMemcpyAsync(&v, h->d_stats.get() + 5, sizeof(v), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, sdpcut_sync(h));
            *value = (int64_t)v;
            return SDPCUT_OK;
        }
        if (h->nn_eval_mode == 1) {
            int64_t skipped = 0;
            const int rc = sdpcut_get_stat(h, SDPCUT_STAT_NN_SKIPPED, &skipped);
            if (rc) return rc;
            *value = h->nn_eval_n - skipped;
            return SDPCUT_OK;
        }
        *value = h->nn_eval_n;
        return SDPCUT_OK;
    case SDPCUT_STAT_NN_SKIPPED:
        if (h->nn_skipped_on_device) {      // a sharded head: its violated count was copied to d_stats[4] behind the selection
            unsigned long long nviol = 0;
            HIP_TRY(h, hipSetDevice(h->device));
            HIP_TRY(h, hipMemcpyAsync(&nviol, h->d_stats.get() + 4, sizeof(nviol), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, sdpcut_sync(h));
            h->stat_nn_skipped = h->nn_skipped_n - (int64_t)nviol;
            h->nn_skipped_on_device = false;
        }
        *value = h->stat_nn_skipped;
        return SDPCUT_OK;
    case SDPCUT_STAT_TIE_SPLITS: *value = h->stat_tie_splits; return SDPCUT_OK;
    case SDPCUT_STAT_INJECTED: *value = h->stat_injected; return SDPCUT_OK;
    case SDPCUT_STAT_POINTS_REDONE: *value = h->stat_points_redone; return SDPCUT_OK;
    case SDPCUT_STAT_DIVERSE_POINTS_FAST: *value = h->stat_diverse_points_fast; return SDPCUT_OK;
    case SDPCUT_STAT_TRI_POINTS_FAST: *value = h->stat_tri_points_fast; return SDPCUT_OK;
    case SDPCUT_STAT_NODE_EVAL_POINTS: *value = h->stat_node_eval_points; return SDPCUT_OK;
    case SDPCUT_STAT_EXACT_HEAD: *value = h->stat_exact_last; return SDPCUT_OK;
    case SDPCUT_STAT_EXACT_GAVE_UP: *value = h->stat_exact_gave_up; return SDPCUT_OK;
    case SDPCUT_STAT_EXACT_RETRIES: *value = h->stat_exact_retries; return SDPCUT_OK;
    case SDPCUT_STAT_SDP_UNCONVERGED: return sdp_unconverged(h, value);
    case SDPCUT_STAT_EMITTED_SELECTIONS: {
        unsigned long long v = 0;
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipMemcpyAsync(&v, h->d_stats.get() + 6, sizeof(v), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, sdpcut_sync(h));
        *value = (int64_t)v;
        return SDPCUT_OK;
    }
    case SDPCUT_STAT_DIRECT_SELECTIONS:
    case SDPCUT_STAT_PF_BIN:
    case SDPCUT_STAT_PF_FLOOR:
    case SDPCUT_STAT_PF_COUNT: {
        unsigned long long v = 0;
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipMemcpyAsync(&v, h->d_stats.get() + (which - SDPCUT_STAT_DIRECT_SELECTIONS), sizeof(v), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, sdpcut_sync(h));
        *value = (int64_t)v;
        return SDPCUT_OK;
    }
    }
    return sdpcut_fail(h, SDPCUT_EINVAL, "unknown statistic");
}

int sdpcut_get_filter_margin(sdpcut_handle h, int k, double *margin)
{
    if (!h || !margin) return SDPCUT_EINVAL;
    if (k < 2 || k > SDPCUT_MAX_K) return sdpcut_fail(h, SDPCUT_EINVAL, "k must be 2..5");
    if (!h->net[k].set) return sdpcut_fail(h, SDPCUT_ESTATE, "no network set for this candidate size");
    *margin = h->net[k].dev.filter_ok ? h->net[k].dev.filter_margin : std::nan("");
    return SDPCUT_OK;
}

// y32_out and (if not null) m_out: the filter's fp32 pass and the margin it decides by, for every candidate of the list
static int filter_audit(sdpcut_handle h, double *y32_out, double *m_out)
{
    SDPCUT_NO_PENDING(h);
    SDPCUT_NO_BOX(h, "sdpcut_filter_audit");
    if (h->N < 1 || h->bucket[3].n != h->N) return sdpcut_fail(h, SDPCUT_ESTATE, "filter audit: the list must hold 3-variable candidates only");
    if (!h->have_point) return sdpcut_fail(h, SDPCUT_ESTATE, "set_point first");
    if (!h->net[3].set || !h->net[3].dev.filter_ok) return sdpcut_fail(h, SDPCUT_ESTATE, "filter audit: the network of 3-variable candidates does not filter");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n = (size_t)h->N;
    DevBuf<double> y;
    HIP_TRY(h, y.reset((m_out ? 2 : 1) * n));
    double *d_y = y.get(), *d_m = m_out ? d_y + n : nullptr;
    int rc = launch_filter_audit(h, d_y, d_m);
    if (!rc && hipMemcpyAsync(y32_out, d_y, n * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess)
        rc = sdpcut_fail(h, SDPCUT_EHIP, "filter audit: copy failed");
    if (!rc && m_out && hipMemcpyAsync(m_out, d_m, n * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess)
        rc = sdpcut_fail(h, SDPCUT_EHIP, "filter audit: copy failed");
    if (!rc && sdpcut_sync(h) != hipSuccess) rc = sdpcut_fail(h, SDPCUT_EHIP, "filter audit: the kernel failed");
    return rc;
}

int sdpcut_filter_audit(sdpcut_handle h, double *y32_out)
{
    if (!h || !y32_out) return SDPCUT_EINVAL;
    return filter_audit(h, y32_out, nullptr);
}

int sdpcut_filter_audit_margins(sdpcut_handle h, double *y32_out, double *m_out)
{
    if (!h || !y32_out || !m_out) return SDPCUT_EINVAL;
    return filter_audit(h, y32_out, m_out);
}

int sdpcut_set_stream(sdpcut_handle h, void *hip_stream)
{
    if (!h) return SDPCUT_EINVAL;
    // the staging copy's transfer lives on the old stream, and its source is host memory the caller may overwrite: a host wait
    if (h->point_inflight) (void)sdpcut_sync(h);
    const hipStream_t next = (hip_stream == SDPCUT_OWN_STREAM) ? h->own_stream : (hipStream_t)hip_stream;
    if (next != h->stream) {
        // Calls that return without waiting (sdpcut_score, sdpcut_set_point_device, ...) may still have work on the old stream that
        // the next call reads the results of: the new stream waits, on the device, for everything enqueued there so far.  Two
        // non-blocking streams are ordered by nothing else.  No host wait; a handle that never switches never comes here.
        HIP_TRY(h, hipSetDevice(h->device));
        if (!h->ev_switch) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_switch, hipEventDisableTiming));
        HIP_TRY(h, hipEventRecord(h->ev_switch, h->stream));
        HIP_TRY(h, hipStreamWaitEvent(next, h->ev_switch, 0));
    }
    h->stream = next;
    h->topk_alt_clean = false;   // its zeroing was ordered on the previous stream only
    return SDPCUT_OK;
}

static __global__ void wake_kernel() {}

int sdpcut_wake(sdpcut_handle h)
{
    if (!h) return SDPCUT_EINVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(wake_kernel, dim3(1), dim3(64), 0, h->stream);
    HIP_TRY(h, hipGetLastError());
    return SDPCUT_OK;
}

int sdpcut_synchronize(sdpcut_handle h)
{
    if (!h) return SDPCUT_EINVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

int sdpcut_last_timing(sdpcut_handle h, double *ms, int n)
{
    if (!h || !ms || n < 1) return SDPCUT_EINVAL;
    if (!h->timing) return sdpcut_fail(h, SDPCUT_ESTATE, "enable SDPCUT_OPT_TIMING first");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, sdpcut_sync(h));
    float a = 0.f, b = 0.f;
    if (!h->timed_score || hipEventElapsedTime(&a, h->ev[0], h->ev[1]) != hipSuccess) a = -1.f;
    if (h->timing < 2 || hipEventElapsedTime(&b, h->ev[2], h->ev[3]) != hipSuccess) b = -1.f;
    (void)hipGetLastError();   // an unrecorded pair is not an error of this library: clear the sticky code
    ms[0] = a;
    if (n > 1) ms[1] = b;
    return SDPCUT_OK;
}

int sdpcut_mfma_probe(sdpcut_handle h, const double *A, const double *B, double *C)
{
    if (!h || !A || !B || !C) return SDPCUT_EINVAL;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = ensure_stage(h, 8 * (64 + 64 + 256));
    if (rc) return rc;
    double *dA = (double *)h->d_stage.get(), *dB = dA + 64, *dC = dB + 64;
    HIP_TRY(h, hipMemcpyAsync(dA, A, 64 * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(dB, B, 64 * 8, hipMemcpyHostToDevice, h->stream));
    rc = launch_mfma_probe(h, dA, dB, dC);
    if (rc) return rc;
    HIP_TRY(h, hipMemcpyAsync(C, dC, 256 * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, sdpcut_sync(h));
    return SDPCUT_OK;
}

} // extern "C"
