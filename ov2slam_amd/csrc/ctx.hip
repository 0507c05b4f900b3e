// ctx.hip -- context, device memory, image batches, pooled pyramid buffers of libov2hip.so
#include "ov2_internal.h"

#include <cstdlib>

ov2_status ov2_set_err(ov2_ctx *ctx, ov2_status s, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) {
        std::lock_guard<std::mutex> g(ctx->mu);
        ctx->err = buf;
    }
    return s;
}

extern "C" const char *ov2_status_string(ov2_status s)
{
    switch (s) {
    case OV2_OK: return "ok";
    case OV2_ERR_INVALID: return "invalid argument";
    case OV2_ERR_HIP: return "HIP runtime error";
    case OV2_ERR_NOMEM: return "out of memory";
    case OV2_ERR_NODEVICE: return "no gfx950 device";
    case OV2_ERR_UNSUPPORTED: return "unsupported";
    default: return "unknown";
    }
}

extern "C" const char *ov2_last_error(const ov2_ctx *ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

extern "C" ov2_status ov2_ctx_create(int device, ov2_ctx **out) { return ov2_ctx_create_ex(device, 0, out); }

// ---- CU share ---------------------------------------------------------------------------------------
// Bit k of a stream's CU mask is compute unit k / OV2_CU_MASK_XCDS of XCD k % OV2_CU_MASK_XCDS: the driver deals the bits
// of a mask round-robin over the XCDs of the device, and an XCD that gets no bit runs on all of its compute units
// (measured with scripts/micro/cu_mask_probe.hip).
extern "C" ov2_status ov2_cu_mask_build(int total_cus, int n_cus, int layout, uint32_t *words_out)
{
    if (!words_out || total_cus <= 0 || n_cus <= 0 || n_cus >= total_cus || (layout != OV2_CU_LAYOUT_SPREAD && layout != OV2_CU_LAYOUT_PACKED))
        return OV2_ERR_INVALID;
    const int words = (total_cus + 31) / 32;
    for (int w = 0; w < words; ++w) words_out[w] = 0;
    int left = n_cus;
    if (layout == OV2_CU_LAYOUT_SPREAD) {
        // dealt evenly: the first n bits visit the XCDs in turn
        for (int k = 0; k < n_cus; ++k) words_out[k >> 5] |= 1u << (k & 31);
        return OV2_OK;
    }
    // packed: every compute unit of XCD 0, then of XCD 1, ...
    for (int x = 0; x < OV2_CU_MASK_XCDS && left > 0; ++x)
        for (int k = x; k < total_cus && left > 0; k += OV2_CU_MASK_XCDS, --left) words_out[k >> 5] |= 1u << (k & 31);
    return OV2_OK;
}

namespace {

constexpr int MAX_DEVICES = 64;
constexpr int MAX_MASK_WORDS = 32;   // 1024 compute units
std::mutex g_live_mu;
int g_live_high[MAX_DEVICES];        // live high-priority contexts of this process per device (under g_live_mu)

struct cu_share_defaults {
    int cus, layout;
};

// OV2_WORKER_CUS (0 = off, or a count) and OV2_WORKER_CU_LAYOUT (0 = spread, 1 = packed) override the built-in default
// share of a normal-priority context that is created beside a high-priority one; read once per process
const cu_share_defaults &worker_cu_defaults()
{
    static const cu_share_defaults d = [] {
        cu_share_defaults v = {OV2_WORKER_CUS_DEFAULT, OV2_WORKER_CU_LAYOUT_DEFAULT};
        if (const char *e = getenv("OV2_WORKER_CUS")) v.cus = atoi(e);
        if (const char *e = getenv("OV2_WORKER_CU_LAYOUT")) v.layout = atoi(e);
        if (v.cus < 0) v.cus = 0;
        if (v.layout != OV2_CU_LAYOUT_SPREAD && v.layout != OV2_CU_LAYOUT_PACKED) v.layout = OV2_WORKER_CU_LAYOUT_DEFAULT;
        return v;
    }();
    return d;
}

int device_cus(int device)
{
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return 0;
    return cus;
}

ov2_status ctx_create(int device, int high_priority, int n_cus, int layout, ov2_ctx **out);

}  // namespace

extern "C" ov2_status ov2_ctx_create_ex(int device, int high_priority, ov2_ctx **out)
{
    // the default rule: a normal-priority context takes the default share while a high-priority context of this process
    // lives on the same device -- it is the one that yields; alone on the device it is never masked
    int n_cus = 0, layout = OV2_CU_LAYOUT_SPREAD;
    if (!high_priority && device >= 0 && device < MAX_DEVICES && worker_cu_defaults().cus > 0) {
        bool beside_high;
        { std::lock_guard<std::mutex> g(g_live_mu); beside_high = g_live_high[device] > 0; }
        if (beside_high && worker_cu_defaults().cus < device_cus(device)) {   // a share the device cannot give is no share
            n_cus = worker_cu_defaults().cus;
            layout = worker_cu_defaults().layout;
        }
    }
    return ctx_create(device, high_priority, n_cus, layout, out);
}

extern "C" ov2_status ov2_ctx_create_cu(int device, int high_priority, int n_cus, int layout, ov2_ctx **out)
{
    if (!out) return OV2_ERR_INVALID;
    *out = nullptr;
    if (n_cus < 0 || (n_cus > 0 && high_priority) || (layout != OV2_CU_LAYOUT_SPREAD && layout != OV2_CU_LAYOUT_PACKED)) return OV2_ERR_INVALID;
    return ctx_create(device, high_priority, n_cus, layout, out);
}

namespace {

ov2_status ctx_create(int device, int high_priority, int n_cus, int layout, ov2_ctx **out)
{
    if (!out) return OV2_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return OV2_ERR_NODEVICE;  // never a CPU fallback
    if (device < 0 || device >= ndev) return OV2_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return OV2_ERR_HIP;
    uint32_t mask[MAX_MASK_WORDS];
    int mask_words = 0, effective_cus = 0;
    if (n_cus > 0) {
        const int total = device_cus(device);
        if (n_cus >= total || total > 32 * MAX_MASK_WORDS || ov2_cu_mask_build(total, n_cus, layout, mask) != OV2_OK) return OV2_ERR_INVALID;
        mask_words = (total + 31) / 32;
        // an XCD the mask gives no bit is not confined: it runs on all of its compute units (header, ov2_ctx_create_cu)
        for (int x = 0; x < OV2_CU_MASK_XCDS; ++x) {
            int bits = 0, own = 0;
            for (int k = x; k < total; k += OV2_CU_MASK_XCDS, ++own) bits += (int)(mask[k >> 5] >> (k & 31) & 1u);
            effective_cus += bits ? bits : own;
        }
    }
    ov2_ctx *c = new ov2_ctx();
    c->device = device;
    c->scratch_dev = nullptr;
    c->scratch_bytes = 0;
    c->tmp_img = nullptr;
    c->ktime_on = false;
    c->wave_prio = high_priority ? OV2_WAVE_PRIO_HIGH : 0;
    c->klt_lanes = 0;
    c->klt_stereo_split = -1;
    c->knn_lanes = 0;
    c->knn_cus = effective_cus;   // compute units the share runs on; 0 (no share): the device's count, read on first use
    c->cu_share = n_cus;
    c->cu_layout = layout;
    c->counts_as_high = false;
    c->lcd_splits = 0;
    c->lcd_calls = 0;
    c->ba_arena = nullptr;
    c->ba_arena_cap = 0;
    c->ba_host = nullptr;
    c->ba_host_cap = 0;
    c->ba_copy_stream = nullptr;
    c->klt_counts[0] = c->klt_counts[1] = nullptr;
    c->klt_counts_words = 0;
    c->klt_counts_cur = 0;
    c->klt_counts_dirty = true;
    c->ba_copy_ev[0] = c->ba_copy_ev[1] = nullptr;
    c->ba_arena2 = nullptr;
    c->ba_arena2_cap = 0;
    c->stage_host = c->stage_dev = nullptr;
    c->stage_cap = 0;
    c->stage_ev = nullptr;
    c->stage_ev_pending = false;
    c->pg_dev = c->pg_pin = c->lpg_dev = nullptr;
    c->pg_dev_cap = c->pg_pin_cap = c->lpg_dev_cap = 0;
    c->pg_ev = nullptr;
    c->pg_ev_pending = false;
    c->stream_kf = nullptr;
    c->kf_scratch_dev = nullptr;
    c->kf_scratch_bytes = 0;
    c->kf.fork = c->kf.done = nullptr;
    c->kf.want_stereo_ev = c->kf.stereo_valid = false;
    // OV2_KF_OVERLAP=0: the keyframe detector chain stays on the main stream (default 1, ov2_ctx_set_kf_overlap)
    const char *kf_env = getenv("OV2_KF_OVERLAP");
    c->kf_overlap = (kf_env ? atoi(kf_env) : 1) > 0 ? 1 : 0;
    // OV2_KF_LAZY_JOIN=0: the detector call joins its chain itself (default 1, ov2_ctx_set_kf_lazy_join)
    const char *lazy_env = getenv("OV2_KF_LAZY_JOIN");
    c->kf_lazy_join = (lazy_env ? atoi(lazy_env) : 1) > 0 ? 1 : 0;
    // OV2_PYR_RING=1..8: depth of the pyramid pool's ring (ov2_ctx_set_pyr_ring); any other value is ignored
    const char *ring_env = getenv("OV2_PYR_RING");
    const int ring = ring_env ? atoi(ring_env) : 0;
    c->pyr_ring = (ring >= 1 && ring <= OV2_PYR_RING_MAX) ? ring : OV2_PYR_RING_DEFAULT;
    c->pyr_alive = 0;
    c->pyr_acquires[0] = c->pyr_acquires[1] = c->pyr_acquires[2] = 0;
    c->pyr_waits[0].store(0);
    c->pyr_waits[1].store(0);
    c->pyr_waits[2].store(0);
    // three streams of one priority: tracking / BA, pyramid builds, keyframe detector chain (a pyramid stream one level
    // more urgent than the other two was measured and changes nothing, DESIGN.md section 7 "A ring for the pyramid pool")
    hipError_t e1, e2, e3;
    if (n_cus > 0) {
        // a CU share: the three streams carry one mask.  The masked create call takes neither a priority nor flags: these
        // are blocking streams of normal priority (include/ov2slam_hip.h, ov2_ctx_create_cu)
        e1 = hipExtStreamCreateWithCUMask(&c->stream.h, (uint32_t)mask_words, mask);
        e2 = hipExtStreamCreateWithCUMask(&c->stream_pyr, (uint32_t)mask_words, mask);
        e3 = hipExtStreamCreateWithCUMask(&c->stream_kf, (uint32_t)mask_words, mask);
    } else {
        int prio_least = 0, prio_greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
        const int prio = high_priority ? prio_greatest : prio_least;
        e1 = hipStreamCreateWithPriority(&c->stream.h, hipStreamNonBlocking, prio);
        e2 = hipStreamCreateWithPriority(&c->stream_pyr, hipStreamNonBlocking, prio);
        e3 = hipStreamCreateWithPriority(&c->stream_kf, hipStreamNonBlocking, prio);
    }
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess ||
        hipEventCreateWithFlags(&c->kf.fork, OV2_ORDER_EVENT_FLAGS) != hipSuccess ||
        hipEventCreateWithFlags(&c->kf.done, OV2_ORDER_EVENT_FLAGS) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreateWithFlags(&c->stage_ev, hipEventDisableTiming) != hipSuccess) {
        if (e1 == hipSuccess) (void)hipStreamDestroy(c->stream.h);
        if (e2 == hipSuccess) (void)hipStreamDestroy(c->stream_pyr);
        if (e3 == hipSuccess) (void)hipStreamDestroy(c->stream_kf);
        delete c;
        return OV2_ERR_HIP;
    }
    if (high_priority && device < MAX_DEVICES) {
        std::lock_guard<std::mutex> g(g_live_mu);
        ++g_live_high[device];
        c->counts_as_high = true;
    }
    *out = c;
    return OV2_OK;
}

}  // namespace

extern "C" void ov2_ctx_destroy(ov2_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->stream_pyr);
    (void)hipStreamSynchronize(c->stream_kf);
    for (ov2_pyr_buf *b : c->pool) ov2_pyr_buf_free(b);
    for (ov2_map *m : c->maps) ov2_map_orphan(m);
    for (ov2_lcd_table *t : c->lcd_tables) ov2_lcd_table_orphan(t);
    if (c->tmp_img) ov2_images_destroy(c->tmp_img);
    for (auto &r : c->ktime_recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    for (auto e : c->ktime_free) (void)hipEventDestroy(e);
    if (c->scratch_dev) (void)hipFree(c->scratch_dev);
    if (c->kf_scratch_dev) (void)hipFree(c->kf_scratch_dev);
    if (c->ba_arena) (void)hipFree(c->ba_arena);
    if (c->ba_host) (void)hipHostFree(c->ba_host);
    for (int i = 0; i < 2; ++i) if (c->klt_counts[i]) (void)hipFree(c->klt_counts[i]);
    if (c->ba_copy_stream) { (void)hipStreamSynchronize(c->ba_copy_stream); (void)hipStreamDestroy(c->ba_copy_stream); }
    for (int i = 0; i < 2; ++i) if (c->ba_copy_ev[i]) (void)hipEventDestroy(c->ba_copy_ev[i]);
    if (c->ba_arena2) (void)hipFree(c->ba_arena2);
    if (c->stage_host) (void)hipHostFree(c->stage_host);
    if (c->stage_dev) (void)hipFree(c->stage_dev);
    (void)hipEventDestroy(c->ev0);
    (void)hipEventDestroy(c->ev1);
    if (c->stage_ev) (void)hipEventDestroy(c->stage_ev);
    if (c->pg_dev) (void)hipFree(c->pg_dev);
    if (c->pg_pin) (void)hipHostFree(c->pg_pin);
    if (c->lpg_dev) (void)hipFree(c->lpg_dev);
    if (c->pg_ev) (void)hipEventDestroy(c->pg_ev);
    if (c->kf.fork) (void)hipEventDestroy(c->kf.fork);
    if (c->kf.done) (void)hipEventDestroy(c->kf.done);
    (void)hipStreamDestroy(c->stream_kf);
    (void)hipStreamDestroy(c->stream_pyr);
    (void)hipStreamDestroy(c->stream.h);
    if (c->counts_as_high) {
        std::lock_guard<std::mutex> g(g_live_mu);
        --g_live_high[c->device];
    }
    delete c;
}

extern "C" ov2_status ov2_ctx_synchronize(ov2_ctx *c)
{
    if (!c) return OV2_ERR_INVALID;
    OV2_HIP(c, hipSetDevice(c->device));   // HIP's current device is per thread
    OV2_HIP(c, hipStreamSynchronize(c->stream_pyr));
    OV2_HIP(c, hipStreamSynchronize(c->stream_kf));
    c->stream.settle(OV2_KFJ_SYNC);   // a pending detector chain has ended with its stream: nothing is left to join
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    return OV2_OK;
}

extern "C" ov2_status ov2_ctx_set_kf_overlap(ov2_ctx *c, int on)
{
    if (!c) return OV2_ERR_INVALID;
    OV2_HIP(c, hipSetDevice(c->device));
    c->stream.join(OV2_KFJ_DEFAULT);   // a chain of the old setting is not left pending under the new one
    c->kf_overlap = on ? 1 : 0;
    return OV2_OK;
}

extern "C" ov2_status ov2_ctx_set_kf_lazy_join(ov2_ctx *c, int on)
{
    if (!c) return OV2_ERR_INVALID;
    OV2_HIP(c, hipSetDevice(c->device));
    c->stream.join(OV2_KFJ_DEFAULT);
    c->kf_lazy_join = on ? 1 : 0;
    return OV2_OK;
}

extern "C" int ov2_ctx_get_kf_lazy_join(const ov2_ctx *c) { return c ? c->kf_lazy_join : -1; }

extern "C" ov2_status ov2_ctx_kf_join_stats(ov2_ctx *c, int64_t out[8])
{
    if (!c || !out) return OV2_ERR_INVALID;
    for (int i = 0; i < OV2_KFJ_N; ++i) out[i] = c->stream.kfj[i].load(std::memory_order_relaxed);
    out[OV2_KFJ_N] = c->stream.pend.done ? 1 : 0;
    return OV2_OK;
}

extern "C" int ov2_kf_ranges_independent(const uintptr_t *rd, int nrd, const uintptr_t *wr, int nwr, const uintptr_t *chain_rd,
                                         int nchain_rd, const uintptr_t *chain_wr, int nchain_wr)
{
    if (nrd < 0 || nwr < 0 || nchain_rd < 0 || nchain_wr < 0 || nrd > 16 || nwr > 16 || nchain_rd > 16 || nchain_wr > 16) return -1;
    if ((nrd && !rd) || (nwr && !wr) || (nchain_rd && !chain_rd) || (nchain_wr && !chain_wr)) return -1;
    ov2_byte_range r[4][16];
    const uintptr_t *src[4] = {rd, wr, chain_rd, chain_wr};
    const int cnt[4] = {nrd, nwr, nchain_rd, nchain_wr};
    for (int k = 0; k < 4; ++k)
        for (int i = 0; i < cnt[k]; ++i) r[k][i] = ov2_range((const void *)src[k][2 * i], (size_t)src[k][2 * i + 1]);
    return ov2_ranges_independent(r[0], nrd, r[1], nwr, r[2], nchain_rd, r[3], nchain_wr) ? 1 : 0;
}

hipStream_t ov2_kf_stream_for(ov2_ctx *c, bool known, const ov2_byte_range *rd, int nrd, const ov2_byte_range *wr, int nwr)
{
    const ov2_kf_pending &p = c->stream.pend;
    if (!p.done) return c->stream;
    if (known && !p.opaque && ov2_ranges_independent(rd, nrd, wr, nwr, p.rd, 4, p.wr, 3)) return c->stream.unjoined();
    c->stream.join(OV2_KFJ_CONFLICT);
    return c->stream;
}

extern "C" ov2_status ov2_ctx_set_wave_prio(ov2_ctx *c, int level)
{
    if (!c) return OV2_ERR_INVALID;
    if (level < 0 || level > 3) return ov2_set_err(c, OV2_ERR_INVALID, "wave priority %d (0..3)", level);
    c->wave_prio = level;
    return OV2_OK;
}

extern "C" int ov2_ctx_get_wave_prio(const ov2_ctx *c) { return c ? c->wave_prio : -1; }

extern "C" int ov2_ctx_get_cu_share(const ov2_ctx *c) { return c ? c->cu_share : -1; }

extern "C" ov2_status ov2_ctx_get_cu_mask(ov2_ctx *c, int words, uint32_t *out)
{
    if (!c || !out || words <= 0) return OV2_ERR_INVALID;
    OV2_HIP(c, hipSetDevice(c->device));
    OV2_HIP(c, hipExtStreamGetCUMask(c->stream.h, (uint32_t)words, out));
    return OV2_OK;
}

void ov2_pyr_buf_free(ov2_pyr_buf *b)
{
    (void)hipEventDestroy(b->ready_ev);
    (void)hipEventDestroy(b->grad_ev);
    (void)hipEventDestroy(b->free_ev);
    (void)hipEventDestroy(b->free_ev2);
    (void)hipEventDestroy(b->free_ev3);
    (void)hipFree(b->base);
    if (b->lut) (void)hipFree(b->lut);
    delete b;
}

// Depth of the pyramid pool's ring: how many released buffers of one geometry whose readers have not finished the pool
// holds before a build takes the oldest of them (and waits for its readers) instead of allocating another one.
extern "C" ov2_status ov2_ctx_set_pyr_ring(ov2_ctx *c, int n)
{
    if (!c) return OV2_ERR_INVALID;
    if (n < 1 || n > OV2_PYR_RING_MAX) return ov2_set_err(c, OV2_ERR_INVALID, "pyramid ring depth %d (1..%d)", n, OV2_PYR_RING_MAX);
    int old;
    { std::lock_guard<std::mutex> g(c->mu); old = c->pyr_ring; c->pyr_ring = n; }
    if (n >= old) return OV2_OK;   // raising frees nothing
    // lowering: every kernel this context enqueued has run once its streams are idle; of each geometry the n buffers
    // released last stay pooled, the older ones are freed
    OV2_HIP(c, hipSetDevice(c->device));
    OV2_HIP(c, hipStreamSynchronize(c->stream_pyr));
    OV2_HIP(c, hipStreamSynchronize(c->stream_kf));
    c->stream.settle(OV2_KFJ_COVERED);
    OV2_HIP(c, hipStreamSynchronize(c->stream.h));
    std::vector<ov2_pyr_buf *> drop;
    {
        std::lock_guard<std::mutex> g(c->mu);
        for (size_t i = c->pool.size(); i-- > 0;) {
            const ov2_pyr_buf *b = c->pool[i];
            int newer = 0;
            for (size_t j = i + 1; j < c->pool.size(); ++j) {
                const ov2_pyr_buf *o = c->pool[j];
                if (o->w == b->w && o->h == b->h && o->pad == b->pad && o->max_level == b->max_level && o->batch == b->batch) ++newer;
            }
            if (newer >= n) {
                drop.push_back(c->pool[i]);
                c->pool.erase(c->pool.begin() + i);
                --c->pyr_alive;
            }
        }
    }
    for (ov2_pyr_buf *b : drop) {
        if (b->has_free_ev2) (void)hipEventSynchronize(b->free_ev2);   // readers another context enqueued on its own stream
        ov2_pyr_buf_free(b);
    }
    return OV2_OK;
}

extern "C" ov2_status ov2_ctx_pyr_pool_stats(ov2_ctx *c, int32_t out[5])
{
    if (!c || !out) return OV2_ERR_INVALID;
    std::lock_guard<std::mutex> g(c->mu);
    out[0] = c->pyr_alive;
    out[1] = (int32_t)c->pool.size();
    out[2] = c->pyr_acquires[0];
    out[3] = c->pyr_acquires[1];
    out[4] = c->pyr_acquires[2];
    return OV2_OK;
}

extern "C" ov2_status ov2_ctx_pyr_wait_stats(ov2_ctx *c, int64_t *issued, int64_t *elided)
{
    if (!c || !issued || !elided) return OV2_ERR_INVALID;
    *issued = c->pyr_waits[0].load(std::memory_order_relaxed);
    *elided = c->pyr_waits[1].load(std::memory_order_relaxed);
    return OV2_OK;
}

extern "C" ov2_status ov2_ctx_pyr_wait_found_complete(ov2_ctx *c, int64_t *found_complete)
{
    if (!c || !found_complete) return OV2_ERR_INVALID;
    *found_complete = c->pyr_waits[2].load(std::memory_order_relaxed);
    return OV2_OK;
}

extern "C" ov2_status ov2_timer_start(ov2_ctx *c)
{
    if (!c) return OV2_ERR_INVALID;
    OV2_HIP(c, hipSetDevice(c->device));   // HIP's current device is per thread
    OV2_HIP(c, hipEventRecord(c->ev0, c->stream));
    return OV2_OK;
}

extern "C" ov2_status ov2_timer_stop(ov2_ctx *c, float *ms)
{
    if (!c || !ms) return OV2_ERR_INVALID;
    OV2_HIP(c, hipSetDevice(c->device));   // HIP's current device is per thread
    c->stream.join(OV2_KFJ_SYNC);   // the interval ends behind a detector chain still pending on the side stream
    OV2_HIP(c, hipEventRecord(c->ev1, c->stream));
    OV2_HIP(c, hipEventSynchronize(c->ev1));
    OV2_HIP(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return OV2_OK;
}

extern "C" ov2_status ov2_dev_alloc(ov2_ctx *c, size_t bytes, void **dptr)
{
    if (!c || !dptr) return OV2_ERR_INVALID;
    OV2_HIP(c, hipSetDevice(c->device));
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 1);
    if (e != hipSuccess) return ov2_set_err(c, OV2_ERR_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    // handed out zeroed: memory the process freed earlier comes back with its old contents otherwise, and rows a kernel
    // leaves unwritten (a detector's output past its count) would depend on what ran before
    OV2_HIP(c, hipMemsetAsync(*dptr, 0, bytes ? bytes : 1, c->stream));
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    return OV2_OK;
}

extern "C" ov2_status ov2_dev_free(ov2_ctx *c, void *dptr)
{
    if (!c) return OV2_ERR_INVALID;
    OV2_HIP(c, hipSetDevice(c->device));   // HIP's current device is per thread
    if (dptr) OV2_HIP(c, hipFree(dptr));
    return OV2_OK;
}

extern "C" ov2_status ov2_memcpy_h2d(ov2_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!c || (bytes && (!dst || !src))) return OV2_ERR_INVALID;
    OV2_HIP(c, hipSetDevice(c->device));   // HIP's current device is per thread
    OV2_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    return OV2_OK;
}

extern "C" ov2_status ov2_memcpy_d2h(ov2_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!c || (bytes && (!dst || !src))) return OV2_ERR_INVALID;
    OV2_HIP(c, hipSetDevice(c->device));   // HIP's current device is per thread
    OV2_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    return OV2_OK;
}

extern "C" ov2_status ov2_memcpy_d2d(ov2_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!c || (bytes && (!dst || !src))) return OV2_ERR_INVALID;
    OV2_HIP(c, hipSetDevice(c->device));   // HIP's current device is per thread
    OV2_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    return OV2_OK;
}

ov2_status ov2_scratch(ov2_ctx *c, size_t bytes, void **out)
{
    if (bytes > c->scratch_bytes) {
        OV2_HIP(c, hipStreamSynchronize(c->stream));
        if (c->scratch_dev) OV2_HIP(c, hipFree(c->scratch_dev));
        c->scratch_dev = nullptr;
        c->scratch_bytes = 0;
        size_t want = bytes + bytes / 2 + 4096;
        hipError_t e = hipMalloc(&c->scratch_dev, want);
        if (e != hipSuccess) return ov2_set_err(c, OV2_ERR_NOMEM, "scratch hipMalloc(%zu)", want);
        c->scratch_bytes = want;
    }
    *out = c->scratch_dev;
    return OV2_OK;
}

ov2_status ov2_kf_scratch(ov2_ctx *c, size_t bytes, void **out)
{
    if (bytes > c->kf_scratch_bytes) {
        OV2_HIP(c, hipStreamSynchronize(c->stream_kf));   // the chain that used the old block; the main stream is left alone
        c->stream.settle(OV2_KFJ_COVERED);                // ... and a chain that was pending has ended
        if (c->kf_scratch_dev) OV2_HIP(c, hipFree(c->kf_scratch_dev));
        c->kf_scratch_dev = nullptr;
        c->kf_scratch_bytes = 0;
        size_t want = bytes + bytes / 2 + 4096;
        hipError_t e = hipMalloc(&c->kf_scratch_dev, want);
        if (e != hipSuccess) return ov2_set_err(c, OV2_ERR_NOMEM, "side scratch hipMalloc(%zu)", want);
        c->kf_scratch_bytes = want;
    }
    *out = c->kf_scratch_dev;
    return OV2_OK;
}

ov2_status ov2_staging(ov2_ctx *c, size_t bytes, void **host, void **dev)
{
    if (c->stage_ev_pending) {   // an asynchronous call left an upload out of the pinned block in flight
        OV2_HIP(c, hipEventSynchronize(c->stage_ev));
        c->stage_ev_pending = false;
    }
    if (bytes > c->stage_cap) {
        OV2_HIP(c, hipStreamSynchronize(c->stream));
        if (c->stage_host) OV2_HIP(c, hipHostFree(c->stage_host));
        if (c->stage_dev) OV2_HIP(c, hipFree(c->stage_dev));
        c->stage_host = c->stage_dev = nullptr;
        c->stage_cap = 0;
        const size_t want = bytes + bytes / 2 + 4096;
        if (hipHostMalloc(&c->stage_host, want, hipHostMallocDefault) != hipSuccess || hipMalloc(&c->stage_dev, want) != hipSuccess)
            return ov2_set_err(c, OV2_ERR_NOMEM, "staging allocation of %zu bytes", want);
        c->stage_cap = want;
    }
    *host = c->stage_host;
    *dev = c->stage_dev;
    return OV2_OK;
}

ov2_status ov2_dev_block(ov2_ctx *c, void **blk, size_t *cap, size_t bytes)
{
    if (bytes <= *cap) return OV2_OK;
    OV2_HIP(c, hipStreamSynchronize(c->stream));   // a queued kernel may still work in the old block
    if (*blk) OV2_HIP(c, hipFree(*blk));
    *blk = nullptr;
    *cap = 0;
    const size_t want = bytes + bytes / 2 + 4096;
    if (hipMalloc(blk, want) != hipSuccess) return ov2_set_err(c, OV2_ERR_NOMEM, "device block of %zu bytes", want);
    *cap = want;
    return OV2_OK;
}

ov2_status ov2_pg_pinned(ov2_ctx *c, size_t bytes, void **host)
{
    if (!c->pg_ev) OV2_HIP(c, hipEventCreateWithFlags(&c->pg_ev, hipEventDisableTiming));
    if (c->pg_ev_pending) {   // the upload of the solve before this one may still be reading the area
        OV2_HIP(c, hipEventSynchronize(c->pg_ev));
        c->pg_ev_pending = false;
    }
    if (bytes > c->pg_pin_cap) {
        if (c->pg_pin) OV2_HIP(c, hipHostFree(c->pg_pin));
        c->pg_pin = nullptr;
        c->pg_pin_cap = 0;
        const size_t want = bytes + bytes / 2 + 4096;
        if (hipHostMalloc(&c->pg_pin, want, hipHostMallocDefault) != hipSuccess)
            return ov2_set_err(c, OV2_ERR_NOMEM, "pinned pose-graph area of %zu bytes", want);
        c->pg_pin_cap = want;
    }
    *host = c->pg_pin;
    return OV2_OK;
}

// ---- images ---------------------------------------------------------------------------------------

extern "C" ov2_status ov2_images_create(ov2_ctx *c, int batch, int w, int h, ov2_images **out)
{
    if (!c || !out || batch <= 0 || w <= 0 || h <= 0) return OV2_ERR_INVALID;
    *out = nullptr;
    OV2_HIP(c, hipSetDevice(c->device));
    ov2_images *im = new ov2_images();
    im->ctx = c;
    im->batch = batch;
    im->w = w;
    im->h = h;
    im->stride = ov2_round_up(w, 64);
    im->bstride = (size_t)im->stride * h;
    hipError_t e = hipMalloc((void **)&im->base, im->bstride * batch);
    if (e != hipSuccess) {
        delete im;
        return ov2_set_err(c, OV2_ERR_NOMEM, "images hipMalloc: %s", hipGetErrorString(e));
    }
    *out = im;
    return OV2_OK;
}

extern "C" ov2_status ov2_images_upload(ov2_ctx *c, ov2_images *im, int b, const uint8_t *host, int stride)
{
    if (!c || !im || !host || b < 0 || b >= im->batch || stride < im->w) return OV2_ERR_INVALID;
    OV2_HIP(c, hipSetDevice(c->device));   // HIP's current device is per thread
    OV2_HIP(c, hipMemcpy2DAsync(im->base + im->bstride * b, im->stride, host, stride, im->w, im->h,
                                hipMemcpyHostToDevice, c->stream));
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    return OV2_OK;
}

extern "C" void ov2_images_destroy(ov2_images *im)
{
    if (!im) return;
    (void)hipFree(im->base);
    delete im;
}

// ---- per-kernel event timing ------------------------------------------------------------------------

const char *ov2_kernel_names[OV2_K_MAX] = {"clahe_lut_kernel", "level0_kernel", "level_kernel", "klt_fb_kernel",
                                           "klt_stage1_kernel", "klt_stage2_kernel",
                                           "ba_eval_kernel", "ba_colnorm_kernel", "ba_scale_kernels", "ba_lmdiag_kernel",
                                           "ba_sinit_kernel", "ba_schur_kernel", "ba_chol_kernel", "ba_backsub_kernel",
                                           "ba_plus_kernel", "ba_flag_kernel", "ba_reduce_kernel", "ba_misc_kernels",
                                           "relpose_kernel", "map_sba_kernel", "detect_cell_kernels", "detect_mask_kernel", "subpix_kernel",
                                           "pnp_kernel", "klt_compact_kernel",
                                           "detect_list_kernels", "map_setup_kernels", "tri_kernel", "stereo_sad_kernel",
                                           "stereo_gate_kernel", "brief_kernel", "match_kernels", "pose_graph_kernel",
                                           "epipolar_kernel", "fivept_dbg_kernel", "p3p_solve_kernel", "p3p_select_kernel",
                                           "p3p_score_kernel", "p3p_final_kernel", "p3p_dbg_kernel", "knn2_kernel",
                                           "loop_match_kernels", "lcd_search_kernel", "lcd_merge_kernel", "lcd_table_kernels",
                                           "fast_score_kernel", "fast_nms_kernel", "fast_select_kernels"};

static hipEvent_t ktime_event(ov2_ctx *c)
{
    if (!c->ktime_free.empty()) {
        hipEvent_t e = c->ktime_free.back();
        c->ktime_free.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

void ov2_ktime_begin(ov2_ctx *c, int id, hipStream_t st)
{
    ov2_ktime_rec r;
    r.id = id;
    r.e0 = ktime_event(c);
    r.e1 = ktime_event(c);
    (void)hipEventRecord(r.e0, st);
    c->ktime_recs.push_back(r);
}

void ov2_ktime_end(ov2_ctx *c, hipStream_t st) { (void)hipEventRecord(c->ktime_recs.back().e1, st); }

extern "C" ov2_status ov2_ktime_enable(ov2_ctx *c, int on)
{
    if (!c) return OV2_ERR_INVALID;
    c->ktime_on = on != 0;
    return OV2_OK;
}

extern "C" ov2_status ov2_ktime_report(ov2_ctx *c, int max_kernels, const char **names, double *total_ms,
                                       long long *launches, int *n_out)
{
    if (!c || !n_out || max_kernels < 0) return OV2_ERR_INVALID;
    OV2_HIP(c, hipStreamSynchronize(c->stream_pyr));
    OV2_HIP(c, hipStreamSynchronize(c->stream_kf));
    c->stream.settle(OV2_KFJ_COVERED);
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    double tot[OV2_K_MAX] = {0};
    long long cnt[OV2_K_MAX] = {0};
    for (auto &r : c->ktime_recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess && r.id >= 0 && r.id < OV2_K_MAX) {
            tot[r.id] += ms;
            cnt[r.id] += 1;
        }
        c->ktime_free.push_back(r.e0);
        c->ktime_free.push_back(r.e1);
    }
    c->ktime_recs.clear();
    int n = 0;
    for (int i = 0; i < OV2_K_MAX && n < max_kernels; ++i) {
        if (!cnt[i]) continue;
        if (names) names[n] = ov2_kernel_names[i] ? ov2_kernel_names[i] : "?";
        if (total_ms) total_ms[n] = tot[i];
        if (launches) launches[n] = cnt[i];
        ++n;
    }
    *n_out = n;
    return OV2_OK;
}

// ---- diagnostics ------------------------------------------------------------------------------------------------
// PMC calibration of the KLT staging pattern (MI355X_MICROARCH.md, HBM: "calibrate on a known byte count in your own
// access pattern"): every lane of a wave loads 16 bytes from a DIFFERENT row (rows `stride` bytes apart, as the KLT
// kernels fetch one window row per lane), column by column, until the whole buffer has been read exactly once.
__global__ __launch_bounds__(64) void dbg_rowload16_kernel(const uint4 *__restrict__ buf, size_t stride16, size_t nrows,
                                                           unsigned *__restrict__ out)
{
    const size_t r = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (r >= nrows) return;
    const uint4 *row = buf + r * stride16;
    unsigned acc = 0;
    for (size_t c = 0; c < stride16; ++c) {
        const uint4 v = row[c];
        acc ^= v.x ^ v.y ^ v.z ^ v.w;
    }
    out[r] = acc;
}

extern "C" ov2_status ov2_dbg_rowload16(ov2_ctx *c, const void *d_buf, size_t stride_bytes, size_t nrows, uint32_t *d_out)
{
    if (!c || !d_buf || !d_out || stride_bytes % 16 || !nrows) return OV2_ERR_INVALID;
    OV2_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(dbg_rowload16_kernel, dim3((unsigned)((nrows + 63) / 64)), dim3(64), 0, c->stream, (const uint4 *)d_buf,
                       stride_bytes / 16, nrows, d_out);
    OV2_HIP(c, hipGetLastError());
    return OV2_OK;
}
