// lcd.hip -- the device word table of the loop detector and its exact search.  ov2_lcd_search2_batch replaces
// obindex2::ImageIndex::searchDescriptors (Thirdparty/obindex2/lib/src/binary_index.cc:217-245, :253-347, two randomised trees walked
// with a budget of 64 checks) by the exact two nearest live words of every query descriptor, B (query set, table) pairs per
// call; the table replaces the descriptor storage of BinaryTree / BinaryDescriptor behind that search.
//
// Two launches whatever B is, no atomics.  The grid of the first is (query blocks of a pair) x (train splits of that pair),
// all pairs in one launch.  A workgroup of 256 threads owns LCD_QPB = 64 consecutive query rows of one pair and one split of
// that pair's table: 4 lanes (a quad) share one query, whose 32 bytes each of them holds in 8 registers, and take the rows
// j, j + 4, ... of a tile.  The rows of the split travel through LDS in tiles of OV2_LCD_TILE rows, beside one word per row
// that is the row's slot, or LCD_NONE when the slot is dead: the key of a row is (distance << 22) | that word, so a dead row's
// key is LCD_NONE and the inner loop has no test for it.  The 16 lanes of a ds_read_b128 group read 4 rows 64 bytes apart,
// which fall on 4 different 4-bank slots for either 16-byte half, so the halves need no swap here (knn.hip, 16 rows).
// Every split writes the two smallest keys of each of its queries to scratch; lcd_merge_kernel, one thread per query row,
// merges the splits of the row.  Keys of one query are distinct (the slot is part of the key; LCD_NONE may repeat), so the
// two smallest of a union do not depend on how the table was split: every split count gives the same bits.
#include <algorithm>

#include "ov2_internal.h"
#include "ov2_wave.h"

struct ov2_lcd_table {
    ov2_ctx *ctx;                   // nullptr once the context is gone (the device side went with it)
    uint4 *rows;                    // cap x 2 uint4
    uint8_t *dead;                  // cap flags
    int cap, n, live;
    int appended;                   // rows appended since the last compaction
    int compactions;
    int32_t next_id;                // word id of the next appended row (never reused)
    std::vector<uint8_t> dead_h;    // host mirror of `dead`, n entries
    std::vector<int32_t> ids;       // word id of every slot, ascending
};

namespace {

enum { LCD_THREADS = 256, LCD_LANES = 4, LCD_QPB = LCD_THREADS / LCD_LANES, LCD_TILE = OV2_LCD_TILE,
       K_LCD_SEARCH = OV2_K_MAP + 16, K_LCD_MERGE = OV2_K_MAP + 17, K_LCD_TABLE = OV2_K_MAP + 18 };
#define LCD_NONE 0x7fffffff       // above every key: dist <= 256 and slot < 1 << 22
#define LCD_MAX_SCRATCH (1 << 26)  // (query row, split) entries of one call

struct lcd_pair {                   // one (query set, table) pair of a call, as the kernels see it
    const uint4 *rows;
    const uint8_t *dead;
    int32_t n;                      // slots of the table
    int32_t q0, nq;                 // first query row, query rows
    int32_t blk0;                   // first workgroup of the pair in the search grid
    int32_t splits, rps;            // train splits, rows per split
    int32_t scr0;                   // first scratch entry; entry of (query row ql, split s) = scr0 + ql * splits + s
    int32_t pad;
};

struct lcd_args {
    int B, total_q;
    const lcd_pair *pairs;
    const uint4 *query;
    int2 *scratch;
    int32_t *idx, *dist;
};

__device__ __forceinline__ int lcd_popc4(const uint4 a, const uint4 b)
{
    return __popc(a.x ^ b.x) + __popc(a.y ^ b.y) + __popc(a.z ^ b.z) + __popc(a.w ^ b.w);
}

__global__ __launch_bounds__(LCD_THREADS) void lcd_search_kernel(const lcd_args A)
{
    __shared__ uint4 tile[LCD_TILE * 2];
    __shared__ int slotv[LCD_TILE];
    const int t = threadIdx.x, sub = t & (LCD_LANES - 1);
    // the last pair whose first workgroup is at or before this one (uniform); pairs without query rows own no workgroup
    int p = 0;
    for (int hi = A.B - 1; p < hi;) {
        const int mid = (p + hi + 1) >> 1;
        if (A.pairs[mid].blk0 <= (int)blockIdx.x) p = mid; else hi = mid - 1;
    }
    const lcd_pair P = A.pairs[p];
    const int local = (int)blockIdx.x - P.blk0;
    const int qb = local / P.splits, s = local - qb * P.splits;
    const int ql = qb * LCD_QPB + t / LCD_LANES;
    const bool mine = ql < P.nq;
    if (qb * LCD_QPB >= P.nq) return;   // whole workgroup (never, by the way the host counts workgroups)
    uint4 qa = make_uint4(0, 0, 0, 0), qc = qa;
    if (mine) { qa = A.query[2 * (size_t)(P.q0 + ql)]; qc = A.query[2 * (size_t)(P.q0 + ql) + 1]; }
    const int r0 = (int)min((long long)s * P.rps, (long long)P.n), r1 = (int)min((long long)r0 + P.rps, (long long)P.n);
    int k0 = LCD_NONE, k1 = LCD_NONE;
    for (int base = r0; base < r1; base += LCD_TILE) {
        const int rows = min((int)LCD_TILE, r1 - base);
        __syncthreads();   // the tile before this one has been read
        for (int i = t; i < 2 * rows; i += LCD_THREADS) tile[i] = P.rows[2 * (size_t)base + i];
        for (int i = t; i < rows; i += LCD_THREADS) slotv[i] = P.dead[base + i] ? LCD_NONE : base + i;
        __syncthreads();
        if (mine) {
#pragma unroll 4
            for (int j = sub; j < rows; j += LCD_LANES) {
                const uint4 ta = tile[2 * j], tb = tile[2 * j + 1];
                const int key = ((lcd_popc4(qa, ta) + lcd_popc4(qc, tb)) << 22) | slotv[j];
                k1 = min(k1, max(k0, key));
                k0 = min(k0, key);
            }
        }
    }
    ov2wave::row_min2_i32<LCD_LANES>(k0, k1);
    if (mine && sub == 0) A.scratch[(size_t)P.scr0 + (size_t)ql * P.splits + s] = make_int2(k0, k1);
}

__global__ __launch_bounds__(LCD_THREADS) void lcd_merge_kernel(const lcd_args A)
{
    const int q = blockIdx.x * LCD_THREADS + threadIdx.x;
    if (q >= A.total_q) return;
    int p = 0;   // the last pair that starts at or before row q and has rows: pairs without rows share their q0 with the next
    for (int hi = A.B - 1; p < hi;) {
        const int mid = (p + hi + 1) >> 1;
        if (A.pairs[mid].q0 <= q) p = mid; else hi = mid - 1;
    }
    while (p > 0 && A.pairs[p].nq == 0) --p;   // trailing pairs without rows
    const lcd_pair P = A.pairs[p];
    const int ql = q - P.q0;
    if (ql < 0 || ql >= P.nq) return;
    const int2 *e = A.scratch + (size_t)P.scr0 + (size_t)ql * P.splits;
    int k0 = LCD_NONE, k1 = LCD_NONE;
    for (int s = 0; s < P.splits; ++s) ov2wave::min2_merge_i32(k0, k1, e[s].x, e[s].y);
    A.idx[2 * (size_t)q] = k0 == LCD_NONE ? -1 : (k0 & 0x3fffff);
    A.dist[2 * (size_t)q] = k0 == LCD_NONE ? -1 : (k0 >> 22);
    A.idx[2 * (size_t)q + 1] = k1 == LCD_NONE ? -1 : (k1 & 0x3fffff);
    A.dist[2 * (size_t)q + 1] = k1 == LCD_NONE ? -1 : (k1 >> 22);
}

__global__ void lcd_kill_kernel(uint8_t *dead, int n_slots, const int32_t *slots, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && slots[i] >= 0 && slots[i] < n_slots) dead[slots[i]] = 1;
}

// dst row first + i = src row src[i], i < n (the stable compaction behind the first dead slot)
__global__ void lcd_gather_kernel(uint4 *dst, const uint4 *rows, const int32_t *src, int first, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // one 16-byte half per thread
    if (i < 2 * n) dst[2 * (size_t)first + i] = rows[2 * (size_t)src[i >> 1] + (i & 1)];
}

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

ov2_status lcd_cus(ov2_ctx *c)
{
    if (!c->knn_cus) {
        int cus = 0;
        OV2_HIP(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
        c->knn_cus = cus > 0 ? cus : 1;
    }
    return OV2_OK;
}

// moves the table into buffers of `cap` slots (device-to-device on the context's stream)
ov2_status lcd_reserve(ov2_ctx *c, ov2_lcd_table *T, int cap)
{
    if (cap <= T->cap) return OV2_OK;
    uint4 *rows = nullptr;
    uint8_t *dead = nullptr;
    if (hipMalloc(&rows, (size_t)cap * 32) != hipSuccess || hipMalloc(&dead, (size_t)cap) != hipSuccess) {
        if (rows) (void)hipFree(rows);
        return ov2_set_err(c, OV2_ERR_NOMEM, "ov2_lcd_table: allocation of %d slots", cap);
    }
    hipStream_t st = c->stream;
    if (T->n) {
        OV2_HIP(c, hipMemcpyAsync(rows, T->rows, (size_t)T->n * 32, hipMemcpyDeviceToDevice, st));
        OV2_HIP(c, hipMemcpyAsync(dead, T->dead, (size_t)T->n, hipMemcpyDeviceToDevice, st));
    }
    OV2_HIP(c, hipStreamSynchronize(st));   // searches and copies that read the old buffers
    if (T->rows) OV2_HIP(c, hipFree(T->rows));
    if (T->dead) OV2_HIP(c, hipFree(T->dead));
    T->rows = rows; T->dead = dead; T->cap = cap;
    return OV2_OK;
}

ov2_status lcd_check(ov2_ctx *c, const ov2_lcd_table *T, const char *who)
{
    if (!c) return OV2_ERR_INVALID;
    if (!T) return ov2_set_err(c, OV2_ERR_INVALID, "%s: null table", who);
    if (T->ctx != c) return ov2_set_err(c, OV2_ERR_INVALID, "%s: the table belongs to another context", who);
    return OV2_OK;
}

// the pairs of a call into `pairs` (B entries); *blocks = workgroups of the search grid, *entries = scratch entries
ov2_status lcd_plan(ov2_ctx *c, int B, ov2_lcd_table *const *tables, const int *n_query, lcd_pair *pairs, long long *blocks,
                    long long *entries, int *total_q)
{
    long long qblocks = 0, nq = 0;
    for (int b = 0; b < B; ++b) {
        if (n_query[b] < 0) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_lcd_search2_batch: negative count");
        ov2_status s = lcd_check(c, tables[b], "ov2_lcd_search2_batch");
        if (s != OV2_OK) return s;
        nq += n_query[b];
        qblocks += (n_query[b] + LCD_QPB - 1) / LCD_QPB;
        if (nq > OV2_LCD_MAX_QUERY) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_lcd_search2_batch: more than %d query rows", OV2_LCD_MAX_QUERY);
    }
    // splits when ov2_lcd_set_splits is 0: four workgroups per compute unit over the whole call, whole tiles per split
    const long long want = qblocks ? (4ll * c->knn_cus + qblocks - 1) / qblocks : 1;
    long long blk = 0, scr = 0, q0 = 0;
    for (int b = 0; b < B; ++b) {
        const ov2_lcd_table *T = tables[b];
        lcd_pair &P = pairs[b];
        P.rows = T->rows; P.dead = T->dead; P.n = T->n; P.q0 = (int32_t)q0; P.nq = n_query[b]; P.pad = 0;
        if (c->lcd_splits) {
            P.splits = c->lcd_splits;
            P.rps = (T->n + P.splits - 1) / P.splits;
        } else {
            const long long tiles = std::max(1, (T->n + LCD_TILE - 1) / LCD_TILE);
            const long long s0 = std::min(std::min(want, tiles), (long long)OV2_LCD_MAX_SPLITS);
            P.rps = (int32_t)((tiles + s0 - 1) / s0) * LCD_TILE;
            P.splits = std::max(1, (T->n + P.rps - 1) / P.rps);
        }
        P.blk0 = (int32_t)blk; P.scr0 = (int32_t)scr;
        blk += (long long)((P.nq + LCD_QPB - 1) / LCD_QPB) * P.splits;
        scr += (long long)P.nq * P.splits;
        q0 += P.nq;
        if (scr > LCD_MAX_SCRATCH)
            return ov2_set_err(c, OV2_ERR_INVALID, "ov2_lcd_search2_batch: %d splits of this many query rows need more than %d scratch entries",
                               P.splits, LCD_MAX_SCRATCH);
    }
    *blocks = blk; *entries = scr; *total_q = (int)nq;
    return OV2_OK;
}

ov2_status lcd_launch(ov2_ctx *c, int B, int total_q, long long blocks, long long entries, const lcd_pair *d_pairs,
                      const uint8_t *d_query, int32_t *d_idx, int32_t *d_dist)
{
    void *scratch = nullptr;
    ov2_status s = ov2_scratch(c, (size_t)entries * sizeof(int2), &scratch);
    if (s != OV2_OK) return s;
    lcd_args A;
    A.B = B; A.total_q = total_q; A.pairs = d_pairs; A.query = (const uint4 *)d_query; A.scratch = (int2 *)scratch;
    A.idx = d_idx; A.dist = d_dist;
    OV2_LAUNCH(c, K_LCD_SEARCH, lcd_search_kernel, dim3((unsigned)blocks), dim3(LCD_THREADS), 0, c->stream, A);
    OV2_LAUNCH(c, K_LCD_MERGE, lcd_merge_kernel, dim3((unsigned)((total_q + LCD_THREADS - 1) / LCD_THREADS)), dim3(LCD_THREADS), 0,
               c->stream, A);
    OV2_HIP(c, hipGetLastError());
    c->lcd_calls++;
    return OV2_OK;
}

ov2_status lcd_search_args(ov2_ctx *c, int B, ov2_lcd_table *const *tables, const int *n_query, const char *who)
{
    if (!c) return OV2_ERR_INVALID;
    if (B < 0) return ov2_set_err(c, OV2_ERR_INVALID, "%s: negative count", who);
    if (B > OV2_LCD_MAX_BATCH) return ov2_set_err(c, OV2_ERR_INVALID, "%s: B %d above %d", who, B, OV2_LCD_MAX_BATCH);
    if (B && (!tables || !n_query)) return ov2_set_err(c, OV2_ERR_INVALID, "%s: null argument", who);
    return OV2_OK;
}

}  // namespace

extern "C" ov2_status ov2_lcd_set_splits(ov2_ctx *c, int splits)
{
    if (!c) return OV2_ERR_INVALID;
    if (splits < 0 || splits > OV2_LCD_MAX_SPLITS)
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_lcd_set_splits: %d is outside 0 .. %d", splits, OV2_LCD_MAX_SPLITS);
    c->lcd_splits = splits;
    return OV2_OK;
}

extern "C" ov2_status ov2_lcd_search_calls(ov2_ctx *c, long long *calls)
{
    if (!c || !calls) return OV2_ERR_INVALID;
    *calls = c->lcd_calls;
    return OV2_OK;
}

extern "C" ov2_status ov2_lcd_table_create(ov2_ctx *c, int capacity_hint, ov2_lcd_table **out)
{
    if (!c) return OV2_ERR_INVALID;
    if (!out) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_lcd_table_create: null argument");
    *out = nullptr;
    if (capacity_hint < 0) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_lcd_table_create: negative count");
    if (capacity_hint > OV2_LCD_MAX_WORDS)
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_lcd_table_create: %d words above %d", capacity_hint, OV2_LCD_MAX_WORDS);
    OV2_HIP(c, hipSetDevice(c->device));
    ov2_lcd_table *T = new ov2_lcd_table();
    T->ctx = c; T->rows = nullptr; T->dead = nullptr;
    T->cap = T->n = T->live = T->appended = T->compactions = 0;
    T->next_id = 0;
    ov2_status s = lcd_reserve(c, T, std::max(capacity_hint, 1024));
    if (s != OV2_OK) { delete T; return s; }
    { std::lock_guard<std::mutex> g(c->mu); c->lcd_tables.push_back(T); }
    *out = T;
    return OV2_OK;
}

void ov2_lcd_table_orphan(ov2_lcd_table *T)
{
    if (T->rows) (void)hipFree(T->rows);
    if (T->dead) (void)hipFree(T->dead);
    T->rows = nullptr; T->dead = nullptr; T->ctx = nullptr;
    T->cap = T->n = T->live = 0;
}

extern "C" void ov2_lcd_table_destroy(ov2_lcd_table *T)
{
    if (!T) return;
    if (ov2_ctx *c = T->ctx) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        { std::lock_guard<std::mutex> g(c->mu); c->lcd_tables.erase(std::remove(c->lcd_tables.begin(), c->lcd_tables.end(), T), c->lcd_tables.end()); }
        ov2_lcd_table_orphan(T);
    }
    delete T;
}

extern "C" ov2_status ov2_lcd_table_count(const ov2_lcd_table *T, int *slots, int *live, int *compactions)
{
    if (!T) return OV2_ERR_INVALID;
    if (slots) *slots = T->n;
    if (live) *live = T->live;
    if (compactions) *compactions = T->compactions;
    return OV2_OK;
}

extern "C" ov2_status ov2_lcd_table_ids(const ov2_lcd_table *T, int cap, int32_t *ids, uint8_t *dead)
{
    if (!T || cap < 0 || (cap && !ids)) return OV2_ERR_INVALID;
    const int n = std::min(cap, T->n);
    if (n) memcpy(ids, T->ids.data(), sizeof(int32_t) * n);
    if (n && dead) memcpy(dead, T->dead_h.data(), n);
    return OV2_OK;
}

extern "C" ov2_status ov2_lcd_table_compact(ov2_ctx *c, ov2_lcd_table *T)
{
    ov2_status s = lcd_check(c, T, "ov2_lcd_table_compact");
    if (s != OV2_OK) return s;
    OV2_HIP(c, hipSetDevice(c->device));
    T->appended = 0;
    if (T->live == T->n) return OV2_OK;   // nothing to move: not counted, the slots keep their meaning
    int first = 0;
    while (!T->dead_h[first]) ++first;    // rows in front of the first dead slot stay where they are
    const int moved = T->live - first;    // live rows behind it (the reference deletes recent words only: few)
    hipStream_t st = c->stream;
    if (moved) {
        // [src | gathered rows]: the rows are gathered into the staging block's device twin and copied back behind `first`
        const size_t o_rows = up256(sizeof(int32_t) * moved), total = o_rows + (size_t)moved * 32;
        char *hp = nullptr, *dp = nullptr;
        s = ov2_staging(c, total, (void **)&hp, (void **)&dp);
        if (s != OV2_OK) return s;
        int32_t *src = (int32_t *)hp;
        for (int i = first, k = 0; i < T->n; ++i)
            if (!T->dead_h[i]) { src[k++] = i; T->ids[first + k - 1] = T->ids[i]; }
        OV2_HIP(c, hipMemcpyAsync(dp, hp, sizeof(int32_t) * moved, hipMemcpyHostToDevice, st));
        OV2_HIP(c, hipEventRecord(c->stage_ev, st));
        c->stage_ev_pending = true;
        OV2_LAUNCH(c, K_LCD_TABLE, lcd_gather_kernel, dim3((unsigned)((2 * moved + 255) / 256)), dim3(256), 0, c->stream,
                   (uint4 *)(dp + o_rows), (const uint4 *)T->rows, (const int32_t *)dp, 0, moved);
        OV2_HIP(c, hipGetLastError());
        OV2_HIP(c, hipMemcpyAsync(T->rows + 2 * (size_t)first, dp + o_rows, (size_t)moved * 32, hipMemcpyDeviceToDevice, st));
    }
    OV2_HIP(c, hipMemsetAsync(T->dead + first, 0, (size_t)(T->n - first), st));
    T->n = T->live;
    T->ids.resize(T->n);
    T->dead_h.assign(T->n, 0);
    T->compactions++;
    return OV2_OK;
}

extern "C" ov2_status ov2_lcd_table_append(ov2_ctx *c, ov2_lcd_table *T, int n, const uint8_t *descs, int *first_slot)
{
    ov2_status s = lcd_check(c, T, "ov2_lcd_table_append");
    if (s != OV2_OK) return s;
    if (n < 0) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_lcd_table_append: negative count");
    if (n && !descs) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_lcd_table_append: null argument");
    if ((long long)T->live + n > OV2_LCD_MAX_WORDS)
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_lcd_table_append: %lld words above %d", (long long)T->live + n, OV2_LCD_MAX_WORDS);
    OV2_HIP(c, hipSetDevice(c->device));
    if ((long long)T->n + n > OV2_LCD_MAX_WORDS) {   // dead slots in the way
        s = ov2_lcd_table_compact(c, T);
        if (s != OV2_OK) return s;
    }
    if (first_slot) *first_slot = T->n;
    if (n == 0) return OV2_OK;
    if (T->n + n > T->cap) {
        s = lcd_reserve(c, T, (int)std::min((long long)OV2_LCD_MAX_WORDS, std::max(2ll * T->cap, (long long)T->n + n)));
        if (s != OV2_OK) return s;
    }
    char *hp = nullptr, *dp = nullptr;
    s = ov2_staging(c, (size_t)n * 32, (void **)&hp, (void **)&dp);
    if (s != OV2_OK) return s;
    memcpy(hp, descs, (size_t)n * 32);
    hipStream_t st = c->stream;
    OV2_HIP(c, hipMemcpyAsync(T->rows + 2 * (size_t)T->n, hp, (size_t)n * 32, hipMemcpyHostToDevice, st));
    OV2_HIP(c, hipEventRecord(c->stage_ev, st));
    c->stage_ev_pending = true;
    OV2_HIP(c, hipMemsetAsync(T->dead + T->n, 0, (size_t)n, st));
    for (int i = 0; i < n; ++i) T->ids.push_back(T->next_id++);
    T->dead_h.insert(T->dead_h.end(), (size_t)n, 0);
    T->n += n; T->live += n; T->appended += n;
    return OV2_OK;
}

extern "C" ov2_status ov2_lcd_table_kill(ov2_ctx *c, ov2_lcd_table *T, int n, const int32_t *slots)
{
    ov2_status s = lcd_check(c, T, "ov2_lcd_table_kill");
    if (s != OV2_OK) return s;
    if (n < 0) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_lcd_table_kill: negative count");
    if (n && !slots) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_lcd_table_kill: null argument");
    for (int i = 0; i < n; ++i)
        if (slots[i] < 0 || slots[i] >= T->n)
            return ov2_set_err(c, OV2_ERR_INVALID, "ov2_lcd_table_kill: slot %d outside 0 .. %d", slots[i], T->n - 1);
    if (n == 0) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    char *hp = nullptr, *dp = nullptr;
    s = ov2_staging(c, sizeof(int32_t) * (size_t)n, (void **)&hp, (void **)&dp);
    if (s != OV2_OK) return s;
    memcpy(hp, slots, sizeof(int32_t) * (size_t)n);
    hipStream_t st = c->stream;
    OV2_HIP(c, hipMemcpyAsync(dp, hp, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    OV2_HIP(c, hipEventRecord(c->stage_ev, st));
    c->stage_ev_pending = true;
    OV2_LAUNCH(c, K_LCD_TABLE, lcd_kill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, T->dead, T->n,
               (const int32_t *)dp, n);
    OV2_HIP(c, hipGetLastError());
    for (int i = 0; i < n; ++i)
        if (!T->dead_h[slots[i]]) { T->dead_h[slots[i]] = 1; T->live--; }
    // More dead slots than live ones: compact.  Each compaction is paid for by the kills since the one before, and it keeps
    // the bound of the header, slots <= 2 live + rows appended since the last compaction (right after a kill, slots <= 2 live).
    if (T->n > 2 * T->live) return ov2_lcd_table_compact(c, T);
    return OV2_OK;
}

extern "C" ov2_status ov2_lcd_search2_batch_dev(ov2_ctx *c, int B, ov2_lcd_table *const *tables, const int *n_query,
                                                const uint8_t *d_query, int32_t *d_idx, int32_t *d_dist)
{
    ov2_status s = lcd_search_args(c, B, tables, n_query, "ov2_lcd_search2_batch_dev");
    if (s != OV2_OK) return s;
    if ((uintptr_t)d_query & 15)   // rows are read 16 bytes at a time
        return ov2_set_err(c, OV2_ERR_INVALID, "ov2_lcd_search2_batch_dev: descriptor arrays must be 16-byte aligned");
    if (B == 0) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    if ((s = lcd_cus(c)) != OV2_OK) return s;
    std::vector<lcd_pair> pairs((size_t)B);
    long long blocks = 0, entries = 0;
    int total_q = 0;
    if ((s = lcd_plan(c, B, tables, n_query, pairs.data(), &blocks, &entries, &total_q)) != OV2_OK) return s;
    if (total_q == 0) return OV2_OK;
    if (!d_query || !d_idx || !d_dist) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_lcd_search2_batch_dev: null array");
    char *hp = nullptr, *dp = nullptr;
    if ((s = ov2_staging(c, sizeof(lcd_pair) * (size_t)B, (void **)&hp, (void **)&dp)) != OV2_OK) return s;
    memcpy(hp, pairs.data(), sizeof(lcd_pair) * (size_t)B);
    hipStream_t st = c->stream;
    OV2_HIP(c, hipMemcpyAsync(dp, hp, sizeof(lcd_pair) * (size_t)B, hipMemcpyHostToDevice, st));
    OV2_HIP(c, hipEventRecord(c->stage_ev, st));
    c->stage_ev_pending = true;
    return lcd_launch(c, B, total_q, blocks, entries, (const lcd_pair *)dp, d_query, d_idx, d_dist);
}

extern "C" ov2_status ov2_lcd_search2_batch(ov2_ctx *c, int B, ov2_lcd_table *const *tables, const int *n_query,
                                            const uint8_t *query, int32_t *idx, int32_t *dist)
{
    ov2_status s = lcd_search_args(c, B, tables, n_query, "ov2_lcd_search2_batch");
    if (s != OV2_OK) return s;
    if (B == 0) return OV2_OK;
    OV2_HIP(c, hipSetDevice(c->device));
    if ((s = lcd_cus(c)) != OV2_OK) return s;
    std::vector<lcd_pair> pairs((size_t)B);
    long long blocks = 0, entries = 0;
    int total_q = 0;
    if ((s = lcd_plan(c, B, tables, n_query, pairs.data(), &blocks, &entries, &total_q)) != OV2_OK) return s;
    if (total_q == 0) return OV2_OK;
    if (!query || !idx || !dist) return ov2_set_err(c, OV2_ERR_INVALID, "ov2_lcd_search2_batch: null array");
    const size_t nq = (size_t)total_q;
    // staging block: [pairs | query || idx | dist]
    const size_t o_q = up256(sizeof(lcd_pair) * (size_t)B), o_idx = o_q + up256(32 * nq), o_dist = o_idx + up256(8 * nq);
    const size_t total = o_dist + up256(8 * nq);
    char *hp = nullptr, *dp = nullptr;
    if ((s = ov2_staging(c, total, (void **)&hp, (void **)&dp)) != OV2_OK) return s;
    memcpy(hp, pairs.data(), sizeof(lcd_pair) * (size_t)B);
    memcpy(hp + o_q, query, 32 * nq);
    hipStream_t st = c->stream;
    OV2_HIP(c, hipMemcpyAsync(dp, hp, o_idx, hipMemcpyHostToDevice, st));
    s = lcd_launch(c, B, total_q, blocks, entries, (const lcd_pair *)dp, (const uint8_t *)(dp + o_q), (int32_t *)(dp + o_idx),
                   (int32_t *)(dp + o_dist));
    if (s != OV2_OK) return s;
    OV2_HIP(c, hipMemcpyAsync(hp + o_idx, dp + o_idx, total - o_idx, hipMemcpyDeviceToHost, st));
    OV2_HIP(c, hipStreamSynchronize(st));
    memcpy(idx, hp + o_idx, 8 * nq);
    memcpy(dist, hp + o_dist, 8 * nq);
    return OV2_OK;
}
