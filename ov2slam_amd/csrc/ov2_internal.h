// ov2_internal.h -- shared state of libov2hip.so (not installed; the public ABI is include/ov2slam_hip.h)
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ov2slam_hip.h"

#define OV2_MAX_LEVELS 8
// left margin of every padded plane, in pixels: >= win (<= 11) and a multiple of 16 so that the interior
// of a row starts 16-byte (u8 plane) / 64-byte (s16x2 plane) aligned for vector loads and stores.
#define OV2_LM 16

struct ov2_level_desc {
    int w, h;             // unpadded size
    int istride;          // bytes per row of the u8 plane (multiple of 64)
    int gstride;          // int16x2 elements per row of the gradient plane (multiple of 16)
    int rows;             // allocated rows = h + 2*pad (+ slack)
    size_t img_off;       // byte offset of image plane of batch 0 inside the allocation
    size_t grad_off;      // byte offset of gradient plane of batch 0
    size_t img_bstride;   // bytes between consecutive batch entries (image plane)
    size_t grad_bstride;  // bytes between consecutive batch entries (gradient plane)
};

// what kernels see (passed by value)
struct ov2_pyr_view {
    int nlevels, pad, batch;
    unsigned char *base;
    ov2_level_desc lv[OV2_MAX_LEVELS];
};

struct ov2_pyr_buf {  // pooled allocation; geometry key = (w,h,pad,max_level,batch)
    int w, h, pad, max_level, batch;
    size_t bytes;
    unsigned char *base;
    unsigned char *lut;  // CLAHE LUTs: batch * tiles * 256 (allocated lazily, max tiles 64x64)
    hipEvent_t ready_ev; // recorded on the ctx pyramid stream when the build is enqueued; consumers wait on it
    // Which build the buffer holds, and the builds the owning ctx's main stream already waits behind: a stream that waited for
    // a build once stays behind it, so a second wait for the same build is an event packet that orders nothing
    // (ov2_pyr_wait_ready).  All three are guarded by the owning ctx's mutex.
    unsigned long long build_seq;         // bumped by every ov2_pyramid_build_images into this buffer
    unsigned long long ready_waited_seq;  // build whose ready_ev the owner's main stream has waited for (or found complete)
    unsigned long long grad_waited_seq;   // build whose gradient planes the owner's main stream is ordered behind
    hipEvent_t free_ev;  // recorded on the ctx main stream when the last handle is released; the next build waits on it
    bool has_free_ev;
    hipEvent_t free_ev2; // recorded on ANOTHER context's main stream by ov2_pyr_release_from (the mapper's readers); the next build waits on it too
    bool has_free_ev2;
    // A detector chain of the owning ctx that reads the buffer from the keyframe side stream: free_ev does not cover it
    // while the main stream has not been put behind the chain (ov2_main_stream::joined_seq < kf_seq), so the release then
    // marks the side stream as well and the next build waits for that mark too.
    unsigned long long kf_seq;   // the last chain of the owning ctx that reads this build (0: none)
    hipEvent_t free_ev3; // recorded on the owning ctx's keyframe side stream when the last handle is released under a pending chain
    bool has_free_ev3;
    // the int16 (Ix, Iy) planes are written on demand (ov2_pyr_need_grad): the 9 x 9 tracking path derives the Scharr
    // values inside its kernel and never reads them.  Both fields are guarded by the owning ctx's mutex.
    bool grad_built;
    hipEvent_t grad_ev;  // recorded behind the kernels that wrote the gradient planes
    ov2_pyr_view view;
};

enum ov2_kernel_id {
    OV2_K_CLAHE_LUT = 0, OV2_K_LEVEL0, OV2_K_LEVEL, OV2_K_KLT_FB, OV2_K_KLT_STAGE1, OV2_K_KLT_STAGE2,
    OV2_K_BA_FIRST,  // BA kernels register from here (ba.hip): 12 ids
    OV2_K_MAP_SBA = 19,  // structure-only BA solver of the map mirrors (map.hip)
    OV2_K_DETECT = 20,
    OV2_K_MAP = 26,  // map mirror scans (map.hip)
    OV2_K_MAX = 48
};
extern const char *ov2_kernel_names[OV2_K_MAX];

struct ov2_byte_range {
    const char *lo, *hi;   // [lo, hi); lo == nullptr: absent
};

static inline ov2_byte_range ov2_range(const void *p, size_t bytes)
{
    return ov2_byte_range{(const char *)p, p ? (const char *)p + bytes : nullptr};
}

static inline bool ranges_meet(const ov2_byte_range &a, const ov2_byte_range &b) { return a.lo && b.lo && a.lo < b.hi && b.lo < a.hi; }

// May a call that reads rd[] and writes wr[] run beside one that reads ord[] and writes owr[]?  Nothing the one writes may
// meet anything the other reads or writes.  An absent range meets nothing: the caller decides what an absent array means.
static inline bool ov2_ranges_independent(const ov2_byte_range *rd, int nrd, const ov2_byte_range *wr, int nwr,
                                          const ov2_byte_range *ord, int nord, const ov2_byte_range *owr, int nowr)
{
    for (int i = 0; i < nwr; ++i) {
        for (int j = 0; j < nord; ++j) if (ranges_meet(wr[i], ord[j])) return false;
        for (int j = 0; j < nowr; ++j) if (ranges_meet(wr[i], owr[j])) return false;
    }
    for (int i = 0; i < nrd; ++i)
        for (int j = 0; j < nowr; ++j) if (ranges_meet(rd[i], owr[j])) return false;
    return true;
}

// ov2_ctx_kf_join_stats: what became of the detector chains started on the keyframe side stream
enum ov2_kf_join_stat {
    OV2_KFJ_STARTED = 0,  // chains enqueued on the side stream
    OV2_KFJ_CONFLICT,     // joined by a tracking / stereo call whose arrays meet the chain's (or could not be proven apart)
    OV2_KFJ_DEFAULT,      // joined by the first other use of the main stream
    OV2_KFJ_SYNC,         // completed by ov2_ctx_synchronize / ov2_timer_stop
    OV2_KFJ_COVERED,      // never joined: the next chain (same stream, same arrays) or a synchronisation of the side stream covered it
    OV2_KFJ_EAGER,        // joined inside the detector call (ov2_ctx_set_kf_lazy_join(0), or a failed launch)
    OV2_KFJ_PYR,          // pyramid builds that waited for a chain still reading the buffer they reuse
    OV2_KFJ_N
};

// A detector chain on the keyframe side stream whose end the main stream has not been put behind (detect.hip).
struct ov2_kf_pending {
    hipEvent_t done = nullptr;           // the chain's end (ov2_kf_fork::done); nullptr: no chain is pending
    unsigned long long seq = 0;          // number of the chain, 1 = the first of the context
    bool opaque = false;                 // an earlier chain on other arrays may still run under this note: no call is proven apart
    ov2_byte_range rd[4], wr[3];         // what the chain reads (thresholds, keypoints, image indices, flags) / writes
                                         //   (thresholds, counts, corners up to out_cap)
};

// The main stream of a context.  It converts to hipStream_t wherever one is expected, and every conversion counts as a use:
// ov2_detect_grid_batch_dev may fork its chain from the event ov2_stereo_matching_dev left in front of its kernels only
// while NOTHING has been enqueued on this stream since (ov2_kf_fork::uses), and a count taken at the one place every
// enqueue passes through cannot miss a call site.  Pure ordering bookkeeping (event records and waits of the pyramid
// pool, which move no data) reads `.h` instead and does not count.
//
// The same place ends a pending detector chain: while one is pending the first conversion puts the stream behind the
// chain's end, so every call is ordered behind the chain exactly as if the detector call had joined it.  Only a call that
// has proven its arrays apart from the chain's (ov2_kf_stream_for) enqueues through unjoined() and leaves the chain
// running beside it.
struct ov2_main_stream {
    hipStream_t h = nullptr;
    mutable std::atomic<unsigned long long> uses{0};
    mutable ov2_kf_pending pend;
    mutable std::atomic<unsigned long long> joined_seq{0};   // the last chain this stream is behind, or that has ended
    mutable std::atomic<long long> kfj[OV2_KFJ_N] = {};
    operator hipStream_t() const
    {
        uses.fetch_add(1, std::memory_order_relaxed);
        if (pend.done) join(OV2_KFJ_DEFAULT);
        return h;
    }
    hipStream_t unjoined() const { uses.fetch_add(1, std::memory_order_relaxed); return h; }
    // puts the stream behind the pending chain (a wait the device cannot take is taken by the host)
    void join(int why) const
    {
        if (!pend.done) return;
        if (hipStreamWaitEvent(h, pend.done, 0) != hipSuccess) (void)hipEventSynchronize(pend.done);
        settle(why);
    }
    // the pending chain has ended, or the stream is behind it: nothing is pending any more
    void settle(int why) const
    {
        if (!pend.done) return;
        joined_seq.store(pend.seq, std::memory_order_release);
        pend.done = nullptr;
        kfj[why].fetch_add(1, std::memory_order_relaxed);
    }
};

// keyframe side stream: the detector chain runs here beside the stereo matching of the same keyframe and, until a call
// needs what it reads or writes, beside the calls that follow (detect.hip; the pending end is ov2_main_stream::pend)
struct ov2_kf_fork {
    hipEvent_t fork, done;               // fork: point of the main stream the chain starts from (recorded by the detector call at
                                         //   the tail, or by ov2_stereo_matching_dev in front of its first kernel); done: end of the
                                         //   chain, waited for by the main stream when a call joins it (ov2_main_stream::join)
    bool want_stereo_ev;                 // set by ov2_stereo_matching_dev for the two-stage tracking call it makes
    bool stereo_valid;                   // `fork` is the stereo call's, and `uses` and the ranges below describe that call
    unsigned long long uses;             // ov2_main_stream::uses right behind that call's last enqueue
    const ov2_pyr_buf *pyr[2];           // the pyramids it reads (image planes: read only)
    ov2_byte_range rd[5], wr[3];         // what it reads (keypoints, priors, flags, image indices, undistorted points) / writes
};

struct ov2_ktime_rec {
    int id;
    hipEvent_t e0, e1;
};

struct ov2_ctx {
    int device;
    ov2_main_stream stream;              // main stream: KLT, detectors, BA
    hipStream_t stream_pyr;              // pyramid builds run here so that frame t+1's pyramid overlaps frame t's KLT
    hipStream_t stream_kf;               // keyframe side stream: the detector chain while kf_overlap is on (always a stream of its own)
    int kf_overlap;                      // ov2_ctx_set_kf_overlap / OV2_KF_OVERLAP: 0 = the chain stays on the main stream
    int kf_lazy_join;                    // ov2_ctx_set_kf_lazy_join / OV2_KF_LAZY_JOIN: 0 = the detector call itself joins its chain
    ov2_kf_fork kf;
    void *kf_scratch_dev;                // scratch of the chain on the side stream (grown on demand; growth waits for
    size_t kf_scratch_bytes;             //   the side stream alone)
    hipEvent_t ev0, ev1;
    std::mutex mu;                       // guards pool + err, and of every pyramid buffer this ctx built: grad_built and the
                                         //   build / waited sequence numbers (held around the event query and wait of ov2_pyr_wait_ready)
    std::vector<ov2_pyr_buf *> pool;     // free pyramid buffers, in release order (oldest first)
    int pyr_ring;                        // ov2_ctx_set_pyr_ring / OV2_PYR_RING: released-but-unfinished buffers of one geometry the
                                         //   pool holds before a build reuses the oldest of them
    int pyr_alive;                       // pyramid buffers allocated and not freed (pooled + handed out); under mu
    int pyr_acquires[3];                 // builds served by a finished / a pending / a newly allocated buffer; under mu
    std::atomic<long long> pyr_waits[3]; // pyramid waits THIS ctx's main stream was asked for: event packets issued / elided /
                                         //   of the elided, those left out because the event had completed (ov2_ctx_pyr_wait_stats,
                                         //   ov2_ctx_pyr_wait_found_complete; atomics, the guard held is the pyramid owner's, not ours)
    std::vector<struct ov2_map *> maps;  // live map mirrors (their device memory is released with the ctx)
    std::string err;
    // scratch for host-pointer entry points (grown on demand)
    void *scratch_dev;
    size_t scratch_bytes;
    ov2_images *tmp_img;                 // staging image for ov2_pyramid_build(host img)
    void *ba_arena;                      // device arena of ov2_ba_solve, grown on demand, kept across solves
    size_t ba_arena_cap;
    void *stage_host, *stage_dev;        // pinned staging block + its device twin for the host-pointer entry points
    size_t stage_cap;
    hipEvent_t stage_ev;                 // recorded behind an asynchronous upload out of the pinned staging block;
    bool stage_ev_pending;               //   ov2_staging waits for it before handing the block out again
    // ov2_pose_graph_solve_batch_dev: descriptors, structure arrays and workspaces of the queued solve in a device block of
    // its own (the staging block may be handed out again while the minimiser is still queued), uploaded from a pinned
    // area that is rewritten only after pg_ev, recorded behind the upload, has passed
    void *pg_dev, *pg_pin;
    size_t pg_dev_cap, pg_pin_cap;
    hipEvent_t pg_ev;
    bool pg_ev_pending;
    // ov2_map_local_pose_graph_batch: the assembled problems (poses | T_ij), result records and skip bytes of the last call
    void *lpg_dev;
    size_t lpg_dev_cap;
    void *ba_arena2;                     // second device block: cell / pair structure of the Schur complement (sized after the build learns the counts)
    size_t ba_arena2_cap;
    void *ba_host;                       // pinned host mirror of the uploaded head of the arena (same offsets)
    size_t ba_host_cap;
    unsigned *klt_counts[2];             // tallies + list lengths of the two-stage KLT, double-buffered: the last kernel of a call
    size_t klt_counts_words;             //   zeroes the OTHER buffer for the next call (no memset in front of every frame)
    int klt_counts_cur;
    bool klt_counts_dirty;               // a call did not run to its end: both buffers are zeroed again
    hipStream_t ba_copy_stream;          // second half of a batch upload (measurements) travels here while the program build sorts
    hipEvent_t ba_copy_ev[2];            // [0] head uploaded (main stream), [1] measurements uploaded (copy stream)
    int wave_prio;                       // ov2_ctx_set_wave_prio: 0..3, the s_setprio level of every kernel this ctx launches that takes one
    int klt_lanes;                       // ov2_klt_set_lanes: 0 = by call size, 3 / 8 / 16 = forced lanes per keypoint
    int klt_stereo_split;                // ov2_klt_set_stereo_split: the level stereoMatching's list B resumes at in the second launch, -1 = built-in
    int knn_lanes;                       // ov2_knn_set_lanes: 0 = by call size, 1 / 4 / 16 / 64 = forced lanes per query
    int knn_cus;                         // compute units the matcher's automatic choice sizes for: the context's CU share, or the
                                         //   device's count (read on first use)
    int cu_share, cu_layout;             // ov2_ctx_create_cu: compute units the three kernel streams are masked to (0 = no mask)
    bool counts_as_high;                 // counted among the live high-priority contexts of its device (the default share rule)
    int lcd_splits;                      // ov2_lcd_set_splits: 0 = by call size, otherwise the forced number of train-axis splits
    long long lcd_calls;                 // ov2_lcd_search2_batch(_dev) calls that launched (ov2_lcd_search_calls)
    std::vector<struct ov2_lcd_table *> lcd_tables;   // live word tables (their device memory is released with the ctx)
    // optional per-kernel hipEvent timing (bench.py roofline leg); off by default
    bool ktime_on;
    std::vector<ov2_ktime_rec> ktime_recs;   // recorded (kernel id, event pair) since the last report
    std::vector<hipEvent_t> ktime_free;      // recycled events
};

struct ov2_images {
    ov2_ctx *ctx;
    int batch, w, h;
    int stride;        // bytes per row (multiple of 64)
    size_t bstride;    // bytes per image
    unsigned char *base;
};

struct ov2_pyr {
    std::atomic<int> refs;
    ov2_ctx *ctx;
    ov2_pyr_buf *buf;
};

// Events that only order streams of one device against each other (the pyramid pool's ready / grad / free marks, the fork
// and join of the keyframe side stream): no timing, and no system-scope fence with the record -- that fence makes the
// writes in front of the event visible to the host and to other devices, and nothing on either reads behind these events.
// stage_ev (the host rewrites the pinned staging block behind it), ba_copy_ev and the timing events keep their flags.
#define OV2_ORDER_EVENT_FLAGS (hipEventDisableTiming | hipEventDisableSystemFence)

#define OV2_PYR_RING_DEFAULT 3   // the smallest depth at which the frame loop no longer waits for its pyramids
#define OV2_PYR_RING_MAX 8

ov2_status ov2_set_err(ov2_ctx *ctx, ov2_status s, const char *fmt, ...);
// frees a pyramid buffer that no kernel reads or writes any more (device memory, LUT, events)
void ov2_pyr_buf_free(ov2_pyr_buf *b);
ov2_status ov2_scratch(ov2_ctx *ctx, size_t bytes, void **out);
// the same for the keyframe side stream's own buffer
ov2_status ov2_kf_scratch(ov2_ctx *ctx, size_t bytes, void **out);
// The main stream for a call that reads rd[] and writes wr[]: while a detector chain is pending and every range is proven
// apart from the chain's, the stream as it is (the chain keeps running beside the call); otherwise the stream behind the
// chain's end.  `known` = false (an array of the call has no known extent) joins as well.
hipStream_t ov2_kf_stream_for(ov2_ctx *ctx, bool known, const ov2_byte_range *rd, int nrd, const ov2_byte_range *wr, int nwr);
// pinned host block of `bytes` and a device block of the same size (grown on demand, kept by the ctx)
ov2_status ov2_staging(ov2_ctx *ctx, size_t bytes, void **host, void **dev);
// a device block the ctx keeps for one purpose (*blk / *cap are its fields), grown on demand behind a synchronisation of
// the main stream; calls that follow each other on that stream may reuse it without one
ov2_status ov2_dev_block(ov2_ctx *ctx, void **blk, size_t *cap, size_t bytes);
// the pinned area the device-pointer pose-graph solve uploads from: handed out once the previous upload out of it has
// passed (the caller records ctx->pg_ev behind its copy and sets pg_ev_pending)
ov2_status ov2_pg_pinned(ov2_ctx *ctx, size_t bytes, void **host);
// posegraph.hip: the batch solve on device-resident poses / T_ij / result records, enqueued on the main stream
ov2_status ov2_pg_solve_dev(ov2_ctx *ctx, const char *who, int B, const ov2_pg_problem *p, const ov2_ba_options *o, ov2_pg_result *d_r);
// ov2_ctx_destroy: free the device side of a map that outlives its ctx (the handle stays valid for ov2_map_destroy)
void ov2_map_orphan(struct ov2_map *m);
// the same for a word table of the loop detector (lcd.hip)
void ov2_lcd_table_orphan(struct ov2_lcd_table *t);

#define OV2_HIP(ctx, call)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return ov2_set_err((ctx), OV2_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                               __FILE__, __LINE__);                                                 \
    } while (0)

// bracket a launch with events when kernel timing is enabled
void ov2_ktime_begin(ov2_ctx *c, int id, hipStream_t st);
void ov2_ktime_end(ov2_ctx *c, hipStream_t st);
// make the ctx main stream wait for the build of `p` (enqueued on the pyramid stream)
ov2_status ov2_pyr_wait_ready(ov2_ctx *c, const ov2_pyr *p);
// ... and, for consumers of the gradient planes, for those planes as well (writes them on c's main stream if no one has yet)
ov2_status ov2_pyr_need_grad(ov2_ctx *c, const ov2_pyr *p);
// klt.hip: two-stage forward-backward tracking (see ov2_klt_tracking_frame_dev); rule33 = 0 for stereo matching
ov2_status ov2_klt_two_stage_dev(ov2_ctx *c, const ov2_pyr *prev, const ov2_pyr *cur, int win, int nlevels_full, int max_iter,
                                 float eps, float err_th, float fb_th, int n, const float *d_kps, const float *d_prior,
                                 const uint8_t *d_has_prior, const int32_t *d_img_idx, float *d_out_xy,
                                 uint8_t *d_out_status, int32_t *d_p3p_req, uint32_t *d_iters, int rule33);
#define OV2_LAUNCH_ON(ctx, id, st, ...)     \
    do {                                    \
        if ((ctx)->ktime_on) ov2_ktime_begin((ctx), (id), (st)); \
        hipLaunchKernelGGL(__VA_ARGS__);    \
        if ((ctx)->ktime_on) ov2_ktime_end((ctx), (st)); \
    } while (0)
#define OV2_LAUNCH(ctx, id, ...) OV2_LAUNCH_ON(ctx, id, (ctx)->stream, __VA_ARGS__)

static inline int ov2_round_up(int v, int m) { return (v + m - 1) / m * m; }
