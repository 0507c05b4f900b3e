// pyramid.hip -- CLAHE + optical-flow pyramid (pyrDown 5x5 + Scharr) for gfx950.
//
// Replaces (reference, /root/reference): VisualFrontEnd::preprocessImage src/visual_front_end.cpp:1143-1177
// = cv::CLAHE::apply + cv::buildOpticalFlowPyramid(img, pyr, Size(9,9), 3); right image src/mapper.cpp:76-81.
// Arithmetic = OpenCV semantics restated in oracle/ov2_oracle_fe.c (integer exact; CLAHE interpolation in
// fp32 with contraction off, v_rndne for cvRound) -- results are bit-identical to the oracle.
//
// HBM layout (one allocation per pyramid batch, see ov2_level_desc): per level a u8 plane and an int16x2
// (Ix,Iy) plane, each padded by `pad` (=win) pixels; the interior of every row starts at column OV2_LM=16
// so that 4-pixel groups are dword (u8) / 16-byte (gradient) aligned.  u8 padding = REFLECT_101, gradient
// padding = 0 (zeroed once when the pooled buffer is created; kernels never write it).
//
// Kernels (all HBM-streaming, byte/int16 work -- no MFMA on purpose):
//   clahe_lut_wave_kernel one wave per (tile, image): LDS histogram -> clip/redistribute -> scan -> LUT
//   level0_kernel         CLAHE bilinear LUT interpolation (or plain copy) -> padded level-0 plane
//   level_kernel          one pass over level l staged in LDS (64x16 tile + 2-px halo):
//                         writes Scharr(l) as 16-byte stores and pyrDown(l) -> level l+1 (+ its reflect border)
#include "ov2_internal.h"
#include "ov2_wave.h"

using ov2wave::reflect101;

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned char sat_u8_rn(float v)
{
    int r = (int)__builtin_rintf(v);  // v_rndne_f32: round half to even == cvRound
    return (unsigned char)min(max(r, 0), 255);
}

// write one u8 pixel of a padded plane together with every REFLECT_101 copy of it in the border.
__device__ __forceinline__ void store_reflections(unsigned char *plane, int istride, int pad, int W, int H, int x,
                                                  int y, unsigned char v, bool write_self)
{
    int xs[3], ys[3], nx = 0, ny = 0;
    xs[nx++] = x;
    if (x >= 1 && x <= pad) xs[nx++] = -x;
    if (x >= W - 1 - pad && x <= W - 2) xs[nx++] = 2 * (W - 1) - x;
    ys[ny++] = y;
    if (y >= 1 && y <= pad) ys[ny++] = -y;
    if (y >= H - 1 - pad && y <= H - 2) ys[ny++] = 2 * (H - 1) - y;
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            if (i == 0 && j == 0 && !write_self) continue;
            plane[(size_t)(ys[j] + pad) * istride + OV2_LM + xs[i]] = v;
        }
}

// ---------------------------------------------------------------------------------------------------
// CLAHE LUT, one WAVE per tile (four tiles per workgroup, no workgroup barrier anywhere): the tile's ~2.6 k pixels are
// 12 dwords per lane, the histogram lives in four interleaved LDS copies private to the wave, lane l owns bins
// 4l .. 4l+3 for the clip / redistribute / scan steps (wave shuffles), and writes its four LUT bytes as one dword.
// A workgroup per tile (the first version) is a chain of barrier-separated phases with eight workgroups resident per CU
// (4.2 rounds for 64 images x 135 tiles); here every tile of the batch is resident at once.
#define CLW_COPIES 4
__global__ __launch_bounds__(256) void clahe_lut_wave_kernel(const unsigned char *__restrict__ src, int w, int h,
                                                             int sstride, size_t sbstride, int tiles_x, int tiles_y,
                                                             int tw, int th, int clip_limit, float lut_scale,
                                                             unsigned char *__restrict__ lut, int wave_prio)
{
    ov2wave::set_wave_prio(wave_prio);
    __shared__ int hist_all[4][256 * CLW_COPIES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int tile = blockIdx.x * 4 + wv, b = blockIdx.y;
    if (tile >= tiles_x * tiles_y) return;           // wave-uniform
    int *hist = hist_all[wv];
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const unsigned char *img = src + sbstride * b;
#pragma unroll
    for (int k = 0; k < 256 * CLW_COPIES / 64 / 4; ++k)
        *reinterpret_cast<int4 *>(&hist[(k * 64 + lane) * 4]) = make_int4(0, 0, 0, 0);
    __builtin_amdgcn_wave_barrier();
    const int x0 = tx * tw, y0 = ty * th, copy = lane & (CLW_COPIES - 1);
    // Tiles of the last tile row / column reach into the REFLECT_101 extension (CLAHE_Impl::apply pads the image to a
    // multiple of the tile grid): an extension pixel is the mirror image of an in-image pixel, so when all mirror sources
    // lie inside this tile's own in-image part (every usual geometry) the tile is histogrammed from that part alone, the
    // mirrored columns / rows counting twice (weights 1, 2, 4) -- the same dword loads as any other tile.
    const int xe = min(x0 + tw, w), ye = min(y0 + th, h);
    const int xm_lo = 2 * w - 1 - x0 - tw, ym_lo = 2 * h - 1 - y0 - th;   // first mirrored column / row (when there is an extension)
    const bool ext_x = x0 + tw > w, ext_y = y0 + th > h;
    if ((!ext_x || (x0 < w - 1 && xm_lo >= x0)) && (!ext_y || (y0 < h - 1 && ym_lo >= y0))) {
        // rows as aligned dwords, pixels of the first / last dword outside [x0, xe) masked
        const int xa = x0 & ~3, ndw = (xe - xa + 3) >> 2;
        const int total = ndw * (ye - y0);
        const unsigned char *base = img + (size_t)y0 * sstride + xa;
        constexpr int CH = 6;
        // the lane's index advances by 64 per load: (row, dword) tracked incrementally instead of divided out
        const int a64 = 64 / ndw, r64 = 64 - a64 * ndw;
        int yy = lane / ndw, dd = lane - yy * ndw;
        for (int i0 = 0; i0 < total; i0 += 64 * CH) {
            unsigned v[CH];
            int xs[CH], ys[CH];
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                const int i = i0 + k * 64 + lane;
                xs[k] = -1000;
                ys[k] = 0;
                v[k] = 0;
                if (i < total) {
                    v[k] = *reinterpret_cast<const unsigned *>(base + (unsigned)(yy * sstride + 4 * dd));
                    xs[k] = xa + 4 * dd - x0;
                    ys[k] = y0 + yy;
                }
                dd += r64; yy += a64;
                if (dd >= ndw) { dd -= ndw; ++yy; }
            }
            if (!ext_x && !ext_y) {   // wave-uniform
#pragma unroll
                for (int k = 0; k < CH; ++k)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if ((unsigned)(xs[k] + j) < (unsigned)tw) atomicAdd(&hist[((v[k] >> (8 * j)) & 255) * CLW_COPIES + copy], 1);
            } else {
#pragma unroll
                for (int k = 0; k < CH; ++k) {
                    const int wy = (ext_y && ys[k] >= ym_lo && ys[k] <= h - 2) ? 2 : 1;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int x = x0 + xs[k] + j;
                        if (x >= x0 && x < xe)
                            atomicAdd(&hist[((v[k] >> (8 * j)) & 255) * CLW_COPIES + copy], (ext_x && x >= xm_lo && x <= w - 2) ? 2 * wy : wy);
                    }
                }
            }
        }
    } else {
        // exotic geometries (an extension wider than the in-image part of its tile): pixel by pixel through the reflection
        const int npx = tw * th;
        for (int i0 = 0; i0 < npx; i0 += 64 * 8) {
            int v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int i = i0 + k * 64 + lane;
                v[k] = -1;
                if (i < npx) {
                    const int yy = i / tw, xx = i - yy * tw;
                    v[k] = img[(size_t)reflect101(y0 + yy, h) * sstride + reflect101(x0 + xx, w)];
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (v[k] >= 0) atomicAdd(&hist[v[k] * CLW_COPIES + copy], 1);
        }
    }
    __builtin_amdgcn_wave_barrier();
    // lane l: bins 4l .. 4l+3
    int hv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int sum = 0;
#pragma unroll
        for (int q = 0; q < CLW_COPIES / 4; ++q) {
            const int4 c = *reinterpret_cast<const int4 *>(&hist[(4 * lane + k) * CLW_COPIES + 4 * q]);
            sum += (c.x + c.y) + (c.z + c.w);
        }
        hv[k] = sum;
    }
    if (clip_limit > 0) {
        int over = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (hv[k] > clip_limit) { over += hv[k] - clip_limit; hv[k] = clip_limit; }
        for (int o = 32; o > 0; o >>= 1) over += __shfl_xor(over, o);
        const int clipped = over;
        const int batch = clipped / 256, residual = clipped - batch * 256;
        // step = 256 / residual and bin / step by float reciprocals: for 0 <= a <= 256 and 1 <= b <= 256,
        // floor(a / b) = (int)((a + 0.5f) * (1.0f / b)) exactly (the true quotient is at least 0.5 / 256 away from an
        // integer boundary, the float error is below 1e-4) -- eight integer divisions of ~25 instructions each per lane gone
        int step = residual ? (int)(256.5f * (1.0f / (float)residual)) : 1;
        if (step < 1) step = 1;
        const float inv_step = 1.0f / (float)step;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int bin = 4 * lane + k;
            hv[k] += batch;
            const int q = (int)(((float)bin + 0.5f) * inv_step);
            if (residual != 0 && bin - q * step == 0 && q < residual) hv[k] += 1;
        }
    }
    // inclusive scan over the 256 bins
    hv[1] += hv[0]; hv[2] += hv[1]; hv[3] += hv[2];
    int tot = hv[3];
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(tot, o);
        if (lane >= o) tot += t;
    }
    const int below = tot - hv[3];
    unsigned outw = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) outw |= (unsigned)sat_u8_rn((float)(hv[k] + below) * lut_scale) << (8 * k);
    reinterpret_cast<unsigned *>(lut + ((size_t)b * tiles_x * tiles_y + tile) * 256)[lane] = outw;
}

// ---------------------------------------------------------------------------------------------------
// level 0: CLAHE interpolation (use_clahe) or copy, 4 px per thread, into the padded plane + reflect border.
// grid (ceil(w/256), h, batch), 64 threads.
__global__ __launch_bounds__(64) void level0_kernel(const unsigned char *__restrict__ src, int w, int h, int sstride,
                                                    size_t sbstride, int use_clahe,
                                                    const unsigned char *__restrict__ lut, int tiles_x, int tiles_y,
                                                    float inv_tw, float inv_th, ov2_pyr_view pv, int wave_prio)
{
    ov2wave::set_wave_prio(wave_prio);
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int y = blockIdx.y, b = blockIdx.z;
    if (x0 >= w) return;
    const ov2_level_desc L = pv.lv[0];
    unsigned char *plane = pv.base + L.img_off + L.img_bstride * b;
    const unsigned char *srow = src + sbstride * b + (size_t)y * sstride;
    unsigned char out[4];
    const int nvalid = min(4, w - x0);
    unsigned int raw = 0;
    if (nvalid == 4) raw = *reinterpret_cast<const unsigned int *>(srow + x0);  // sstride, x0 multiples of 4
    else for (int i = 0; i < nvalid; ++i) raw |= (unsigned int)srow[x0 + i] << (8 * i);

    if (use_clahe) {
        const float tyf = (float)y * inv_th - 0.5f;
        int ty1 = (int)floorf(tyf);
        int ty2 = ty1 + 1;
        const float ya = tyf - (float)ty1;
        const float ya1 = 1.0f - ya;
        ty1 = max(ty1, 0);
        ty2 = min(ty2, tiles_y - 1);
        const unsigned char *p1 = lut + ((size_t)b * tiles_y + ty1) * tiles_x * 256;
        const unsigned char *p2 = lut + ((size_t)b * tiles_y + ty2) * tiles_x * 256;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int x = x0 + i;
            const float txf = (float)x * inv_tw - 0.5f;
            int tx1 = (int)floorf(txf);
            int tx2 = tx1 + 1;
            const float xa = txf - (float)tx1;
            const float xa1 = 1.0f - xa;
            tx1 = max(tx1, 0);
            tx2 = min(tx2, tiles_x - 1);
            const int v = (raw >> (8 * i)) & 255;
            const int i1 = tx1 * 256 + v, i2 = tx2 * 256 + v;
            const float res = ((float)p1[i1] * xa1 + (float)p1[i2] * xa) * ya1 +
                              ((float)p2[i1] * xa1 + (float)p2[i2] * xa) * ya;
            out[i] = sat_u8_rn(res);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = (unsigned char)((raw >> (8 * i)) & 255);
    }
    unsigned char *drow = plane + (size_t)(y + pv.pad) * L.istride + OV2_LM;
    if (nvalid == 4) {
        *reinterpret_cast<unsigned int *>(drow + x0) =
            (unsigned int)out[0] | ((unsigned int)out[1] << 8) | ((unsigned int)out[2] << 16) | ((unsigned int)out[3] << 24);
    } else {
        for (int i = 0; i < nvalid; ++i) drow[x0 + i] = out[i];
    }
    const bool yedge = (y <= pv.pad) || (y >= h - 1 - pv.pad);
    const bool xedge = (x0 <= pv.pad) || (x0 + 3 >= w - 1 - pv.pad);
    if (yedge || xedge)
        for (int i = 0; i < nvalid; ++i) store_reflections(plane, L.istride, pv.pad, w, h, x0 + i, y, out[i], false);
}

// ---------------------------------------------------------------------------------------------------
// level 0, CLAHE path, tiled: one workgroup = 64 x 64 px, the <= (64/tw+3) x (64/th+3) tile LUTs that its pixels
// interpolate between are staged in LDS once (3 KB for EuRoC geometry) instead of 16 L1/L2 byte gathers per thread.
// Same arithmetic as level0_kernel (which remains the fallback for exotic tile geometries and the copy path).
__global__ __launch_bounds__(256) void level0_clahe_tiled_kernel(const unsigned char *__restrict__ src, int w, int h,
                                                                 int sstride, size_t sbstride,
                                                                 const unsigned char *__restrict__ lut, int tiles_x,
                                                                 int tiles_y, float inv_tw, float inv_th, int ncx_max,
                                                                 ov2_pyr_view pv, int wave_prio)
{
    ov2wave::set_wave_prio(wave_prio);
    // tile = 64 x 64 px; a thread owns 4 px in each of 4 rows (y0+ty, +16, +32, +48) and issues its 4 source loads
    // back to back: the kernel is bound by the number of memory round trips per resident wave, not by bandwidth.
    extern __shared__ __attribute__((aligned(16))) unsigned char llds[];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 64;
    const int xl = min(x0 + 63, w - 1), yl = min(y0 + 63, h - 1);
    const int cx_lo = max((int)floorf((float)x0 * inv_tw - 0.5f), 0);
    const int cx_hi = min((int)floorf((float)xl * inv_tw - 0.5f) + 1, tiles_x - 1);
    const int cy_lo = max((int)floorf((float)y0 * inv_th - 0.5f), 0);
    const int cy_hi = min((int)floorf((float)yl * inv_th - 0.5f) + 1, tiles_y - 1);
    const int ncx = cx_hi - cx_lo + 1, ncy = cy_hi - cy_lo + 1;
    const int x = x0 + 4 * (tid & 15), ty = tid >> 4;
    const int nvalid = min(4, w - x);
    const unsigned char *sb = src + sbstride * b;
    unsigned int raw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = y0 + ty + 16 * k;
        raw[k] = 0;
        if (x < w && y < h) {
            const unsigned char *srow = sb + (size_t)y * sstride;
            if (nvalid == 4) raw[k] = *reinterpret_cast<const unsigned int *>(srow + x);
            else for (int i = 0; i < nvalid; ++i) raw[k] |= (unsigned int)srow[x + i] << (8 * i);
        }
    }
    const unsigned char *lb = lut + (size_t)b * tiles_x * tiles_y * 256;
    for (int i = tid; i < ncx * ncy * 64; i += 256) {   // dwords
        const int t = i >> 6, d = i & 63;
        const int cy = t / ncx, cx = t - cy * ncx;
        reinterpret_cast<unsigned int *>(llds)[(cy * ncx_max + cx) * 64 + d] =
            reinterpret_cast<const unsigned int *>(lb + ((size_t)(cy_lo + cy) * tiles_x + cx_lo + cx) * 256)[d];
    }
    __syncthreads();
    if (x >= w) return;
    const ov2_level_desc L = pv.lv[0];
    unsigned char *plane = pv.base + L.img_off + L.img_bstride * b;
    // the x interpolation terms are shared by the 4 rows
    float xa[4], xa1[4];
    int o1[4], o2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float txf = (float)(x + i) * inv_tw - 0.5f;
        int tx1 = (int)floorf(txf);
        int tx2 = tx1 + 1;
        xa[i] = txf - (float)tx1;
        xa1[i] = 1.0f - xa[i];
        tx1 = max(tx1, 0);
        tx2 = min(tx2, tiles_x - 1);
        o1[i] = min(max(tx1 - cx_lo, 0), ncx - 1) * 256;
        o2[i] = min(max(tx2 - cx_lo, 0), ncx - 1) * 256;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = y0 + ty + 16 * k;
        if (y >= h) break;
        const float tyf = (float)y * inv_th - 0.5f;
        int ty1 = (int)floorf(tyf);
        int ty2 = ty1 + 1;
        const float ya = tyf - (float)ty1;
        const float ya1 = 1.0f - ya;
        ty1 = max(ty1, 0);
        ty2 = min(ty2, tiles_y - 1);
        const unsigned char *p1 = llds + (size_t)(ty1 - cy_lo) * ncx_max * 256;
        const unsigned char *p2 = llds + (size_t)(ty2 - cy_lo) * ncx_max * 256;
        unsigned char out[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = (raw[k] >> (8 * i)) & 255;
            const int i1 = o1[i] + v, i2 = o2[i] + v;
            const float res = ((float)p1[i1] * xa1[i] + (float)p1[i2] * xa[i]) * ya1 + ((float)p2[i1] * xa1[i] + (float)p2[i2] * xa[i]) * ya;
            out[i] = sat_u8_rn(res);
        }
        unsigned char *drow = plane + (size_t)(y + pv.pad) * L.istride + OV2_LM;
        if (nvalid == 4) {
            *reinterpret_cast<unsigned int *>(drow + x) =
                (unsigned int)out[0] | ((unsigned int)out[1] << 8) | ((unsigned int)out[2] << 16) | ((unsigned int)out[3] << 24);
        } else {
            for (int i = 0; i < nvalid; ++i) drow[x + i] = out[i];
        }
        const bool yedge = (y <= pv.pad) || (y >= h - 1 - pv.pad);
        const bool xedge = (x <= pv.pad) || (x + 3 >= w - 1 - pv.pad);
        if (yedge || xedge)
            for (int i = 0; i < nvalid; ++i) store_reflections(plane, L.istride, pv.pad, w, h, x + i, y, out[i], false);
    }
}

// ---------------------------------------------------------------------------------------------------
// level l -> Scharr(l) [+ pyrDown -> level l+1].  Tile 64x16 px of level l, 256 threads.
// grid (ceil(w/64), ceil(h/16), batch).
#define TILE_W 64
// 64 rows per workgroup: a thread owns 4 Scharr groups and 4 pyrDown outputs, so each resident wave carries several
// memory round trips' worth of work (with 16-row tiles the kernel was bound by round trips per wave, not bandwidth)
#define TILE_H 16
#define LDS_ROWS (TILE_H + 4)  // rows y0-2 .. y0+TILE_H+1
#define LDS_DW 18              // dwords per row: cols x0-4 .. x0+67

__global__ __launch_bounds__(256) void level_kernel(ov2_pyr_view pv, int l, int has_next, int do_scharr, int wave_prio)
{
    ov2wave::set_wave_prio(wave_prio);
    __shared__ unsigned int tile[LDS_ROWS][LDS_DW];
    const int tid = threadIdx.x;
    const int b = blockIdx.z;
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;
    const ov2_level_desc L = pv.lv[l];
    const int pad = pv.pad;
    const unsigned char *img = pv.base + L.img_off + L.img_bstride * b;

    // stage: dword loads from the padded plane (border already holds REFLECT_101, so no index logic)
    for (int i = tid; i < LDS_ROWS * LDS_DW; i += 256) {
        const int r = i / LDS_DW, c = i - r * LDS_DW;
        int row = y0 - 2 + r + pad;                       // padded row index
        row = min(row, L.h + 2 * pad - 1);                // tiles hanging over the bottom edge
        int dw = (OV2_LM + x0 - 4) / 4 + c;               // dword column
        dw = min(dw, L.istride / 4 - 1);                  // tiles hanging over the right edge
        tile[r][c] = *reinterpret_cast<const unsigned int *>(img + (size_t)row * L.istride + 4 * dw);
    }
    __syncthreads();

    // ---- Scharr: 4 px per thread ------------------------------------------------------------------
    if (do_scharr)
    for (int rr = 0; rr < TILE_H / 16; ++rr) {
        const int tx = tid & 15, ty = (tid >> 4) + 16 * rr;
        const int x = x0 + 4 * tx, y = y0 + ty;
        if (y < L.h && x < L.w) {
            // bytes x-4 .. x+7 of rows y-1,y,y+1  ->  need cols x-1 .. x+4
            int t0[6], t1[6];
            unsigned int ra[3], rb[3], rc[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                ra[k] = tile[ty + 1][tx + k];
                rb[k] = tile[ty + 2][tx + k];
                rc[k] = tile[ty + 3][tx + k];
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const int byte = 3 + c;  // col x-1 is byte 3 of the 12 loaded
                const int a = (ra[byte >> 2] >> (8 * (byte & 3))) & 255;
                const int m = (rb[byte >> 2] >> (8 * (byte & 3))) & 255;
                const int d = (rc[byte >> 2] >> (8 * (byte & 3))) & 255;
                t0[c] = (a + d) * 3 + m * 10;
                t1[c] = d - a;
            }
            short g[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                g[2 * i] = (short)(t0[i + 2] - t0[i]);
                g[2 * i + 1] = (short)((t1[i] + t1[i + 2]) * 3 + t1[i + 1] * 10);
            }
            short *grow = reinterpret_cast<short *>(pv.base + L.grad_off + L.grad_bstride * b) +
                          ((size_t)(y + pad) * L.gstride + OV2_LM + x) * 2;
            if (x + 3 < L.w) {
                uint4 v;
                v.x = (unsigned short)g[0] | ((unsigned int)(unsigned short)g[1] << 16);
                v.y = (unsigned short)g[2] | ((unsigned int)(unsigned short)g[3] << 16);
                v.z = (unsigned short)g[4] | ((unsigned int)(unsigned short)g[5] << 16);
                v.w = (unsigned short)g[6] | ((unsigned int)(unsigned short)g[7] << 16);
                *reinterpret_cast<uint4 *>(grow) = v;
            } else {
                for (int i = 0; i < L.w - x; ++i) { grow[2 * i] = g[2 * i]; grow[2 * i + 1] = g[2 * i + 1]; }
            }
        }
    }

    // ---- pyrDown: 32 x (TILE_H/2) outputs per tile, TILE_H/16 per thread -----------------------------------
    if (has_next)
    for (int rr = 0; rr < TILE_H / 16; ++rr) {
        const ov2_level_desc N = pv.lv[l + 1];
        const int lx = tid & 31, ly = (tid >> 5) + 8 * rr;
        const int xo = (x0 >> 1) + lx, yo = (y0 >> 1) + ly;
        const int c0 = 2 + 2 * lx;  // first byte (col 2xo-2) inside the LDS row
        int acc = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const unsigned int d0 = tile[2 * ly + j][c0 >> 2], d1 = tile[2 * ly + j][(c0 >> 2) + 1];
            const unsigned long long v = (((unsigned long long)d1 << 32) | d0) >> (8 * (c0 & 3));
            const int p0 = (int)(v & 255), p1 = (int)((v >> 8) & 255), p2 = (int)((v >> 16) & 255),
                      p3 = (int)((v >> 24) & 255), p4 = (int)((v >> 32) & 255);
            const int r = p0 + p4 + 4 * (p1 + p3) + 6 * p2;
            const int kj = (j == 0 || j == 4) ? 1 : ((j == 2) ? 6 : 4);
            acc += kj * r;
        }
        const unsigned int val = (unsigned int)((acc + 128) >> 8);
        // pack 4 neighbouring outputs into one dword store where the group is complete
        const unsigned int v1 = __shfl_down(val, 1), v2 = __shfl_down(val, 2), v3 = __shfl_down(val, 3);
        unsigned char *nplane = pv.base + N.img_off + N.img_bstride * b;
        const bool valid = xo < N.w && yo < N.h;
        const int gx = xo & ~3;  // group origin
        const bool full = (gx + 3 < N.w) && yo < N.h;
        if (full) {
            if ((lx & 3) == 0)
                *reinterpret_cast<unsigned int *>(nplane + (size_t)(yo + pad) * N.istride + OV2_LM + xo) =
                    val | (v1 << 8) | (v2 << 16) | (v3 << 24);
        } else if (valid) {
            nplane[(size_t)(yo + pad) * N.istride + OV2_LM + xo] = (unsigned char)val;
        }
        if (valid) {
            const bool edge = (xo <= pad) || (xo >= N.w - 1 - pad) || (yo <= pad) || (yo >= N.h - 1 - pad);
            if (edge) store_reflections(nplane, N.istride, pad, N.w, N.h, xo, yo, (unsigned char)val, false);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// pyrDown alone (what a build runs: the Scharr planes are written on demand).  Tile = 128 x 32 px of level l in LDS
// (+ 2-px halo, rows as dwords from the column 4 left of the tile), a thread owns FOUR adjacent outputs: per source row
// one 16-byte LDS read holds the 11 pixels they touch, the 5 x 5 binomial is applied as 1-4-6-4-1 along the row and
// down the five rows (exact integers), and the four results leave as one dword store.  Same arithmetic as
// level_kernel's pyrDown part (oracle: pyr_down_rows); grid (ceil(w/128), ceil(h/32), batch), 256 threads.
#define PD_TW 128
#define PD_TH 32
#define PD_ROWS (PD_TH + 4)       // rows y0-2 .. y0+PD_TH+1
#define PD_DW (PD_TW / 4 + 4)     // dwords per row: cols x0-4 .. x0+PD_TW+11

__global__ __launch_bounds__(256) void pyrdown_kernel(ov2_pyr_view pv, int l, int wave_prio)
{
    ov2wave::set_wave_prio(wave_prio);
    __shared__ __attribute__((aligned(16))) unsigned int tile[PD_ROWS][PD_DW];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int x0 = blockIdx.x * PD_TW, y0 = blockIdx.y * PD_TH;
    const ov2_level_desc L = pv.lv[l], N = pv.lv[l + 1];
    const int pad = pv.pad;
    const unsigned char *img = pv.base + L.img_off + L.img_bstride * b;
    for (int i = tid; i < PD_ROWS * PD_DW; i += 256) {
        const int r = i / PD_DW, c = i - r * PD_DW;
        const int row = min(y0 - 2 + r + pad, L.h + 2 * pad - 1);            // tiles hanging over the bottom edge
        const int dw = min((OV2_LM + x0 - 4) / 4 + c, L.istride / 4 - 1);    // ... and over the right edge
        tile[r][c] = *reinterpret_cast<const unsigned int *>(img + (size_t)row * L.istride + 4 * dw);
    }
    __syncthreads();
    // thread -> outputs (xo .. xo+3, yo): 16 groups per output row, 16 output rows
    const int gx = tid & 15, ly = tid >> 4;
    const int xo = (x0 >> 1) + 4 * gx, yo = (y0 >> 1) + ly;
    if (yo >= N.h || xo >= N.w) return;
    int acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        // source columns 2 xo - 2 .. 2 xo + 8 = bytes 2 .. 12 of the 16 bytes from LDS column 8 gx (tile column 0 = x0 - 4);
        // output o takes bytes 2 + 2o .. 6 + 2o: v_dot4_u32_u8 with (1, 4, 6, 4) on the first four, the fifth as addend
        const uint4 q = *reinterpret_cast<const uint4 *>(&tile[2 * ly + j][2 * gx]);
        const unsigned d0 = __builtin_amdgcn_alignbyte(q.y, q.x, 2), d2 = __builtin_amdgcn_alignbyte(q.z, q.y, 2);
        const unsigned wts = 0x04060401u;
        int r[4];
        r[0] = (int)__builtin_amdgcn_udot4(d0, wts, (q.y >> 16) & 255u, false);
        r[1] = (int)__builtin_amdgcn_udot4(q.y, wts, q.z & 255u, false);
        r[2] = (int)__builtin_amdgcn_udot4(d2, wts, (q.z >> 16) & 255u, false);
        r[3] = (int)__builtin_amdgcn_udot4(q.z, wts, q.w & 255u, false);
        const int kj = (j == 0 || j == 4) ? 1 : ((j == 2) ? 6 : 4);
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[o] += kj * r[o];
    }
    unsigned char out[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) out[o] = (unsigned char)((acc[o] + 128) >> 8);
    unsigned char *nplane = pv.base + N.img_off + N.img_bstride * b;
    unsigned char *dp = nplane + (size_t)(yo + pad) * N.istride + OV2_LM + xo;
    const int nv = min(4, N.w - xo);
    if (nv == 4) *reinterpret_cast<unsigned int *>(dp) = (unsigned)out[0] | ((unsigned)out[1] << 8) | ((unsigned)out[2] << 16) | ((unsigned)out[3] << 24);
    else for (int o = 0; o < nv; ++o) dp[o] = out[o];
    const bool edge = (xo <= pad) || (xo + 3 >= N.w - 1 - pad) || (yo <= pad) || (yo >= N.h - 1 - pad);
    if (edge)
        for (int o = 0; o < nv; ++o) store_reflections(nplane, N.istride, pad, N.w, N.h, xo + o, yo, out[o], false);
}

// ---------------------------------------------------------------------------------------------------
// TWO pyrDowns in one launch: level l -> l+1 -> l+2, with no hand-off between workgroups.  A workgroup owns a
// P2_TW x P2_TH tile of level l+2 and the level-(l+1) block [2X, 2X + 2 P2_TW) x [2Y, 2Y + 2 P2_TH) under it (the blocks
// partition level l+1).  It stages level l for that block and the ring both binomials reach into, forms level l+1 over
// the block plus a 2-px ring in LDS (the ring is recomputed by the neighbouring workgroups), writes the block's own
// pixels, and forms its level-(l+2) tile from LDS.  Ring positions outside level l+1 take the value of their
// REFLECT_101 source pixel (what the padded plane holds there), copied inside LDS from the in-image part; level-l reads
// past the padded plane clamp and feed only those positions.  Arithmetic = pyrdown_kernel's.
//   LDS level l:   rows 4Y-6 .. 4Y+4 P2_TH+4, columns from 4X-16 (16-byte loads; 16-byte aligned in the plane)
//   LDS level l+1: rows 2Y-2 .. 2Y+2 P2_TH+1, groups of four columns from 2X-4 (group g = columns 2X-4+4g .. +3)
// grid (ceil(w_{l+2}/P2_TW), ceil(h_{l+2}/P2_TH), batch), 256 threads.
static_assert(OV2_LM % 16 == 0, "pyrdown2_kernel stages 16-byte chunks from column -16 of the tile");
#define P2_TW 32
#define P2_TH 16
#define P2_R1 (2 * P2_TH + 4)                  // level-(l+1) rows in LDS
#define P2_G1 (P2_TW / 2 + 2)                  // level-(l+1) dword groups per LDS row (the first and last feed the ring)
#define P2_DW1 ((P2_G1 + 3) & ~3)              // level-(l+1) LDS row stride, dwords (16-byte rows)
#define P2_R0 (2 * P2_R1 + 3)                  // level-l rows in LDS
#define P2_Q0 ((2 * P2_G1 + 3 + 3) / 4)        // level-l 16-byte chunks per LDS row (group g reads dwords 2g+1 .. 2g+4)
#define P2_DW0 (4 * P2_Q0)

// four pyrDown outputs, packed: q[j] = 16 bytes of source row j whose bytes 2 .. 12 are columns 2 xo - 2 .. 2 xo + 8
__device__ __forceinline__ unsigned pyr_down4(const uint4 (&q)[5])
{
    int acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        // output o takes bytes 2 + 2o .. 6 + 2o: v_dot4_u32_u8 with (1, 4, 6, 4) on the first four, the fifth as addend
        const unsigned d0 = __builtin_amdgcn_alignbyte(q[j].y, q[j].x, 2), d2 = __builtin_amdgcn_alignbyte(q[j].z, q[j].y, 2);
        const unsigned wts = 0x04060401u;
        int r[4];
        r[0] = (int)__builtin_amdgcn_udot4(d0, wts, (q[j].y >> 16) & 255u, false);
        r[1] = (int)__builtin_amdgcn_udot4(q[j].y, wts, q[j].z & 255u, false);
        r[2] = (int)__builtin_amdgcn_udot4(d2, wts, (q[j].z >> 16) & 255u, false);
        r[3] = (int)__builtin_amdgcn_udot4(q[j].z, wts, q[j].w & 255u, false);
        const int kj = (j == 0 || j == 4) ? 1 : ((j == 2) ? 6 : 4);
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[o] += kj * r[o];
    }
    return (unsigned)((acc[0] + 128) >> 8) | ((unsigned)((acc[1] + 128) >> 8) << 8) |
           ((unsigned)((acc[2] + 128) >> 8) << 16) | ((unsigned)((acc[3] + 128) >> 8) << 24);
}

// four packed pixels at (x, y) of level N (x a multiple of 4, inside the level); the border copies leave in lds_border
__device__ __forceinline__ void store_group(unsigned char *plane, const ov2_level_desc &N, int pad, int x, int y, unsigned v)
{
    unsigned char *dp = plane + (size_t)(y + pad) * N.istride + OV2_LM + x;
    const int nv = min(4, N.w - x);
    if (nv == 4) *reinterpret_cast<unsigned int *>(dp) = v;
    else for (int o = 0; o < nv; ++o) dp[o] = (unsigned char)(v >> (8 * o));
}

// the REFLECT_101 copies of a block's own pixels (x0 .. x0+BW-1, y0 .. y0+bh-1, clipped to the level) in the plane's border,
// from the block in LDS (pixel (x, y) at src[(y - y0) * sstride + x - x0]): the mirrored rows of own rows (dwords over the
// own columns, bytes where a dword straddles the right edge), then the mirrored columns of own and mirrored rows (bytes,
// consecutive lanes on consecutive columns of one row).  Same targets as store_reflections applied to every own pixel, in
// a few coalesced passes instead of scattered byte stores per pixel (those cost pyrdown2_kernel 6 of its 17 us).
template <int BW>
__device__ __forceinline__ void lds_border(const unsigned char *src, int sstride, int w, int h, int bh, unsigned char *plane,
                                           int istride, int pad, int x0, int y0)
{
    const int tid = threadIdx.x;
    const int xe = min(x0 + BW, w), ye = min(y0 + bh, h), nown = ye - y0;
    const int t_lo = max(y0, 1), nT = max(min(ye - 1, pad) - t_lo + 1, 0);                  // rows -> -y
    const int b_lo = max(y0, h - 1 - pad), nB = max(min(ye - 1, h - 2) - b_lo + 1, 0);      // rows -> 2 (h-1) - y
    const int l_lo = max(x0, 1), nL = max(min(xe - 1, pad) - l_lo + 1, 0);
    const int r_lo = max(x0, w - 1 - pad), nR = max(min(xe - 1, w - 2) - r_lo + 1, 0);
    const int nmy = nT + nB, nmx = nL + nR;
    for (int i = tid; i < nmy * (BW / 4); i += 256) {
        const int m = i / (BW / 4), c = i - m * (BW / 4), x = x0 + 4 * c;
        if (x >= w) continue;
        const int ys = m < nT ? t_lo + m : b_lo + m - nT, Y = m < nT ? -ys : 2 * (h - 1) - ys;
        const unsigned char *sp = src + (ys - y0) * sstride + 4 * c;
        unsigned char *dp = plane + (size_t)(Y + pad) * istride + OV2_LM + x;
        if (x + 3 < w) *reinterpret_cast<unsigned int *>(dp) = *reinterpret_cast<const unsigned int *>(sp);
        else for (int o = 0; o < w - x; ++o) dp[o] = sp[o];
    }
    for (int i = tid; i < (nown + nmy) * nmx; i += 256) {
        const int ri = i / nmx, ci = i - ri * nmx;
        const int m = ri - nown;
        const int ys = m < 0 ? y0 + ri : (m < nT ? t_lo + m : b_lo + m - nT);
        const int Y = m < 0 ? ys : (m < nT ? -ys : 2 * (h - 1) - ys);
        const int xs = ci < nL ? l_lo + ci : r_lo + ci - nL, X = ci < nL ? -xs : 2 * (w - 1) - xs;
        plane[(size_t)(Y + pad) * istride + OV2_LM + X] = src[(ys - y0) * sstride + xs - x0];
    }
}

__global__ __launch_bounds__(256) void pyrdown2_kernel(ov2_pyr_view pv, int l, int wave_prio)
{
    ov2wave::set_wave_prio(wave_prio);
    __shared__ __attribute__((aligned(16))) unsigned int t0[P2_R0][P2_DW0];
    __shared__ __attribute__((aligned(16))) unsigned int t1[P2_R1][P2_DW1];
    __shared__ __attribute__((aligned(16))) unsigned int t2[P2_TH][P2_TW / 4];   // the level-(l+2) tile, for its border
    const int tid = threadIdx.x, b = blockIdx.z;
    const int X = blockIdx.x * P2_TW, Y = blockIdx.y * P2_TH;
    const ov2_level_desc L = pv.lv[l], N = pv.lv[l + 1], M = pv.lv[l + 2];
    const int pad = pv.pad;
    const unsigned char *img = pv.base + L.img_off + L.img_bstride * b;
    // all of a thread's loads in flight together (a guarded load per trip made each trip wait for the previous one): the
    // last trip's surplus threads repeat the last chunk, the same bytes to the same place
    constexpr int NLD = (P2_R0 * P2_Q0 + 255) / 256;
    uint4 ld[NLD];
    int lo[NLD];
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
        const int i = min(tid + 256 * k, P2_R0 * P2_Q0 - 1);
        const int r = i / P2_Q0, c = i - r * P2_Q0;
        const int row = min(max(4 * Y - 6 + r + pad, 0), L.h + 2 * pad - 1);          // pad < 6: the top ring clamps
        const int q = min((OV2_LM + 4 * X - 16) / 16 + c, L.istride / 16 - 1);        // tiles hanging over the right edge
        ld[k] = *reinterpret_cast<const uint4 *>(img + (size_t)row * L.istride + 16 * q);
        lo[k] = r * P2_DW0 + 4 * c;
    }
#pragma unroll
    for (int k = 0; k < NLD; ++k) *reinterpret_cast<uint4 *>(&t0[0][0] + lo[k]) = ld[k];
    __syncthreads();
    // ---- level l+1 over the block and its ring; the block's own groups (1 .. P2_TW/2, rows 2 .. 2 P2_TH+1) also to HBM
    unsigned char *nplane = pv.base + N.img_off + N.img_bstride * b;
    for (int it = tid; it < P2_R1 * P2_G1; it += 256) {
        const int r = it / P2_G1, g = it - r * P2_G1;
        uint4 q[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const unsigned int *p = &t0[2 * r + j][2 * g + 1];
            q[j] = make_uint4(p[0], p[1], p[2], p[3]);
        }
        const unsigned v = pyr_down4(q);
        t1[r][g] = v;
        const int x1 = 2 * X - 4 + 4 * g, y1 = 2 * Y - 2 + r;
        if (g >= 1 && g <= P2_TW / 2 && r >= 2 && r < 2 + 2 * P2_TH && x1 < N.w && y1 < N.h) store_group(nplane, N, pad, x1, y1, v);
    }
    __syncthreads();
    // the level-(l+1) border copies of the block's own pixels (reads own pixels only: no barrier against the pass below)
    if (2 * X <= pad || 2 * X + 2 * P2_TW - 1 >= N.w - 1 - pad || 2 * Y <= pad || 2 * Y + 2 * P2_TH - 1 >= N.h - 1 - pad)
        lds_border<2 * P2_TW>(reinterpret_cast<const unsigned char *>(&t1[2][1]), 4 * P2_DW1, N.w, N.h, 2 * P2_TH, nplane, N.istride,
                              pad, 2 * X, 2 * Y);
    // ---- ring positions outside level l+1 (columns -2, -1, w, w+1 over the LDS rows; rows -2, -1, h, h+1 over the LDS
    // columns) <- their REFLECT_101 source pixel.  Every source lies inside the level and inside this block's LDS region
    // (2X <= w - 1, so w - 3 >= 2X - 2), and no source is a target: one pass.
    if (X == 0 || 2 * X + 2 * P2_TW + 2 > N.w || Y == 0 || 2 * Y + 2 * P2_TH + 2 > N.h) {   // workgroup-uniform
        unsigned char *b1 = reinterpret_cast<unsigned char *>(&t1[0][0]);
        const int xlo = 2 * X - 2, xhi = 2 * X + 2 * P2_TW + 1, ylo = 2 * Y - 2, yhi = 2 * Y + 2 * P2_TH + 1;   // needed ring
        for (int i = tid; i < 4 * P2_R1 + 4 * 4 * P2_G1; i += 256) {
            int x1, y1;
            if (i < 4 * P2_R1) {
                const int k = i / P2_R1;
                y1 = ylo + (i - k * P2_R1);
                x1 = k < 2 ? k - 2 : N.w + k - 2;
            } else {
                const int j = i - 4 * P2_R1, k = j / (4 * P2_G1);
                x1 = 2 * X - 4 + (j - k * 4 * P2_G1);
                y1 = k < 2 ? k - 2 : N.h + k - 2;
            }
            if (x1 < max(xlo, -2) || x1 > min(xhi, N.w + 1) || y1 < max(ylo, -2) || y1 > min(yhi, N.h + 1)) continue;
            const int rx = reflect101(x1, N.w), ry = reflect101(y1, N.h);
            b1[(y1 - ylo) * 4 * P2_DW1 + x1 - (2 * X - 4)] = b1[(ry - ylo) * 4 * P2_DW1 + rx - (2 * X - 4)];
        }
        __syncthreads();
    }
    // ---- level l+2: P2_TW / 4 groups of four outputs x P2_TH rows
    unsigned char *mplane = pv.base + M.img_off + M.img_bstride * b;
    for (int it = tid; it < (P2_TW / 4) * P2_TH; it += 256) {
        const int gx = it % (P2_TW / 4), ly = it / (P2_TW / 4);
        const int xo = X + 4 * gx, yo = Y + ly;
        if (yo >= M.h || xo >= M.w) continue;
        uint4 q[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) q[j] = *reinterpret_cast<const uint4 *>(&t1[2 * ly + j][2 * gx]);
        const unsigned v = pyr_down4(q);
        t2[ly][gx] = v;
        store_group(mplane, M, pad, xo, yo, v);
    }
    if (X <= pad || X + P2_TW - 1 >= M.w - 1 - pad || Y <= pad || Y + P2_TH - 1 >= M.h - 1 - pad) {   // workgroup-uniform
        __syncthreads();
        lds_border<P2_TW>(reinterpret_cast<const unsigned char *>(&t2[0][0]), P2_TW, M.w, M.h, P2_TH, mplane, M.istride, pad, X, Y);
    }
}

// ---------------------------------------------------------------------------------------------------
// level 0 (CLAHE path) AND the first pyrDown in one pass: the workgroup forms the CLAHE output of a 128 x 60 px tile
// plus the 2-px ring the 5 x 5 binomial reaches into (64 rows x 34 dwords, columns x0-4 .. x0+131), keeps it in LDS,
// writes the tile's own pixels to the level-0 plane (128-byte rows: whole lines) and then runs pyrdown_kernel's
// arithmetic from LDS -- level 0 is not read back, one launch tail less.  Ring positions outside the image take the value
// of their REFLECT_101 source pixel, which is what the padded plane holds there.
// The interpolation makes ONE LDS read per pixel: for every interpolation cell the tile touches (the rectangle between
// four neighbouring tile centres; <= 4 x 3 for EuRoC geometry) the four surrounding LUTs are interleaved into a
// 256-entry table of byte quads, so a pixel value fetches all four taps with one dword read (v_cvt_f32_ubyte0..3 unpack
// them); the per-pixel arithmetic is the expression of level0_kernel evaluated two taps at a time by the packed fp32
// instructions (each product and sum rounded separately), so the bytes are the same.
// The kernel is bound by vector instruction issue, so everything that is not per pixel is hoisted out of the pixel loop:
//   - a lane owns one dword column (4 px) for the whole tile: its reflected columns, x weights and quad-table cell
//     offsets are computed once;
//   - per staged row, the reflected source row, the y weights and the cell row live in a 16-byte LDS record (one per
//     lane of each wave, the wave's own copy), read with one ds_read_b128 whose address is an immediate offset;
//   - a wave works on row PAIRS (lanes 0-31 / 32-63 = own dword columns 1..32 of rows 2p, 2p+1), so the 30 own pairs
//     and the 2 halo pairs are 8 per wave; the halo dword columns 0 and 33 of the 64 rows are a short pass of waves 0, 1;
//   - edge tiles differ only in how a lane loads its four source bytes (two dwords + v_perm with a per-lane selector
//     instead of one dword); the reflected copies of the plane border leave in a pass after the tile is complete.
#define L0_TW 128
#define L0_TH 60                 // even: the level-1 rows of a tile start at y0 / 2
#define L0_ROWS (L0_TH + 4)      // staged rows y0-2 .. y0+L0_TH+1 = one row record per lane (the last row feeds nothing)
#define L0_DW 36                 // LDS row stride in dwords (16-byte aligned rows for the pyrDown's uint4 reads); 0..33 used
#define L0_RT_DW (4 * L0_ROWS)   // one wave's row records, dwords

struct l0_cols {                 // one lane's four pixel columns
    float xa[4], xa1[4];
    unsigned cellx[4];           // byte offset of the pixel's cell column in the quad tables
    unsigned ws, sel;            // edge loads: 8-byte window start and the v_perm selector of the four bytes in it
};

__device__ __forceinline__ void l0_col_meta(int x, int w, float inv_tw, int txA, int ncellx, l0_cols &m)
{
    int xr[4], lo = w - 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        xr[i] = min(max(reflect101(x + i, w), 0), w - 1);
        lo = min(lo, xr[i]);
        const float txf = (float)xr[i] * inv_tw - 0.5f;
        const float fl = floorf(txf);
        m.xa[i] = txf - fl;
        m.xa1[i] = 1.0f - m.xa[i];
        m.cellx[i] = (unsigned)min(max((int)fl - txA, 0), ncellx - 1) * 1024u;
    }
    // the reflected bytes of a dword column that feeds an output span at most 8 bytes from their 4-aligned start; capping the
    // start at the last full dword pair keeps both loads inside the row (the image stride is a multiple of 64 >= w).  Columns
    // that feed nothing (far right of the last block) get clamped, in-bounds garbage.
    m.ws = (unsigned)min(lo & ~3, ((w - 1) & ~3) - 4);
    m.sel = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) m.sel |= ((unsigned)(xr[i] - (int)m.ws) & 7u) << (8 * i);
}

template <bool COLS_IN>
__device__ __forceinline__ unsigned l0_load(const unsigned char *__restrict__ sb, unsigned rowoff, int x, const l0_cols &m)
{
    if (COLS_IN) return *reinterpret_cast<const unsigned int *>(sb + (rowoff + (unsigned)x));
    const unsigned int *p = reinterpret_cast<const unsigned int *>(sb + (rowoff + m.ws));
    return __builtin_amdgcn_perm(p[1], p[0], m.sel);
}

// four CLAHE pixels of one staged dword; rec = the row record (1 - ya, ya, cell row offset, source row offset)
__device__ __forceinline__ unsigned l0_interp(unsigned raw, const l0_cols &m, uint4 rec, const unsigned char *qb)
{
    const v2f yw = {__uint_as_float(rec.x), __uint_as_float(rec.y)};
    unsigned int rb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // ((tl xa1 + tr xa) ya1 + (bl xa1 + br xa) ya), every product and sum rounded on its own, two at a time
        // (v_pk_mul_f32 / v_pk_add_f32); the result lies in [0, 255], so adding 2^23 leaves cvRound(res) in the
        // low mantissa byte (round-to-nearest-even, like v_rndne)
        const unsigned q = *reinterpret_cast<const unsigned int *>(qb + (rec.z + m.cellx[i] + 4u * ((raw >> (8 * i)) & 255u)));
        const v2f left = {(float)(q & 255u), (float)((q >> 16) & 255u)}, right = {(float)((q >> 8) & 255u), (float)(q >> 24)};
        const v2f xl = {m.xa1[i], m.xa1[i]}, xr2 = {m.xa[i], m.xa[i]};
        const v2f tb = (left * xl + right * xr2) * yw;
        rb[i] = __float_as_uint((tb.x + tb.y) + 8388608.0f);
    }
    return __builtin_amdgcn_perm(__builtin_amdgcn_perm(rb[3], rb[2], 0x0c0c0400u),
                                 __builtin_amdgcn_perm(rb[1], rb[0], 0x0c0c0400u), 0x05040100u);
}

// the own dword columns 1..32 of the 64 staged rows (row pairs p = wave + 4 k), own pixels stored to the level-0 plane
template <bool COLS_IN>
__device__ __forceinline__ void l0_rows(const unsigned char *__restrict__ sb, int w, int h, unsigned char *__restrict__ plane,
                                        int istride, int pad, float inv_tw, int txA, int ncellx, int x0, int y0,
                                        unsigned int (*tile)[L0_DW], const uint4 *rt, const unsigned char *qb)
{
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, cl = lane & 31, x = x0 + 4 * cl;
    l0_cols m;
    l0_col_meta(x, w, inv_tw, txA, ncellx, m);
    const uint4 *rl = rt + 2 * wv + half;                 // row 2 p + half = 2 wv + half + 8 k
    unsigned int raw[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) raw[k] = l0_load<COLS_IN>(sb, rl[8 * k].w, x, m);   // all rows' loads in flight together
    __syncthreads();   // quad tables complete
    const bool xin = x < w;
    const bool yfull = y0 + L0_TH <= h;
    unsigned char *pl = plane + (unsigned)((y0 - 2 + pad + 2 * wv + half) * istride + OV2_LM + x);
    unsigned int *tl = &tile[2 * wv + half][1 + cl];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int p = wv + 4 * k;
        const unsigned packed = l0_interp(raw[k], m, rl[8 * k], qb);
        // a dword of an own column that straddles the right edge holds the reflections of columns w .. w+2 (< w + pad)
        if (p >= 1 && p <= L0_TH / 2 && xin && (yfull || y0 - 2 + 2 * p + half < h))
            *reinterpret_cast<unsigned int *>(pl + (unsigned)(8 * k * istride)) = packed;
        tl[8 * k * L0_DW] = packed;
    }
}

// the REFLECT_101 copies of the tile's own pixels in the level-0 plane's border, from the finished LDS tile: the mirrored rows
// of own rows (dwords over the own columns) and the mirrored columns of own and mirrored rows (bytes); same targets as
// store_reflections applied to every own pixel
__device__ __forceinline__ void l0_border(int w, int h, unsigned char *__restrict__ plane, int istride, int pad, int x0, int y0,
                                          const unsigned int (*tile)[L0_DW])
{
    const int tid = threadIdx.x;
    const int xe = min(x0 + L0_TW, w), ye = min(y0 + L0_TH, h), nown = ye - y0;
    const int t_lo = max(y0, 1), nT = max(min(ye - 1, pad) - t_lo + 1, 0);                  // rows -> -y
    const int b_lo = max(y0, h - 1 - pad), nB = max(min(ye - 1, h - 2) - b_lo + 1, 0);      // rows -> 2 (h-1) - y
    const int l_lo = max(x0, 1), nL = max(min(xe - 1, pad) - l_lo + 1, 0);
    const int r_lo = max(x0, w - 1 - pad), nR = max(min(xe - 1, w - 2) - r_lo + 1, 0);
    const int nmy = nT + nB, nmx = nL + nR;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int i = tid; i < nmy * 32; i += 256) {
        const int m = i >> 5, c = i & 31, x = x0 + 4 * c;
        if (x >= w) continue;
        const int ys = m < nT ? t_lo + m : b_lo + m - nT, Y = m < nT ? -ys : 2 * (h - 1) - ys;
        *reinterpret_cast<unsigned int *>(plane + (unsigned)((Y + pad) * istride + OV2_LM + x)) = tile[ys - y0 + 2][1 + c];
    }
    if (nmx == 0) return;
    // item -> (row, column) through a float reciprocal: i < 92 * 32, so floor((i + 0.5) / nmx) is exact
    const float inv = 1.0f / (float)nmx;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int i = tid; i < (nown + nmy) * nmx; i += 256) {
        const int ri = (int)(((float)i + 0.5f) * inv), ci = i - ri * nmx;
        const int m = ri - nown;
        const int ys = m < 0 ? y0 + ri : (m < nT ? t_lo + m : b_lo + m - nT);
        const int Y = m < 0 ? ys : (m < nT ? -ys : 2 * (h - 1) - ys);
        const int xs = ci < nL ? l_lo + ci : r_lo + ci - nL, X = ci < nL ? -xs : 2 * (w - 1) - xs;
        plane[(unsigned)((Y + pad) * istride + OV2_LM + X)] = reinterpret_cast<const unsigned char *>(tile[ys - y0 + 2])[xs - x0 + 4];
    }
}

__global__ __launch_bounds__(256) void level0_clahe_pyrdown_kernel(const unsigned char *__restrict__ src, int w, int h,
                                                                   int sstride, size_t sbstride,
                                                                   const unsigned char *__restrict__ lut, int tiles_x,
                                                                   int tiles_y, float inv_tw, float inv_th, ov2_pyr_view pv, int wave_prio)
{
    ov2wave::set_wave_prio(wave_prio);
    extern __shared__ __attribute__((aligned(16))) unsigned int fl[];
    unsigned int (*tile)[L0_DW] = reinterpret_cast<unsigned int (*)[L0_DW]>(fl);   // L0_ROWS x L0_DW
    uint4 *rt_all = reinterpret_cast<uint4 *>(fl + L0_ROWS * L0_DW);              // 4 waves x L0_ROWS row records
    unsigned int *quad = fl + L0_ROWS * L0_DW + 4 * L0_RT_DW;                      // cells x 256 byte quads
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), b = blockIdx.z;
    const int x0 = blockIdx.x * L0_TW, y0 = blockIdx.y * L0_TH;
    const int pad = pv.pad;
    const int xmin = max(x0 - 4, 0), xmax = min(x0 + L0_TW + 3, w - 1);
    const int ymin = max(y0 - 2, 0), ymax = min(y0 + L0_TH + 1, h - 1);
    const int txA = (int)floorf((float)xmin * inv_tw - 0.5f), txB = (int)floorf((float)xmax * inv_tw - 0.5f);
    const int tyA = (int)floorf((float)ymin * inv_th - 0.5f), tyB = (int)floorf((float)ymax * inv_th - 0.5f);
    const int ncellx = txB - txA + 1, ncelly = tyB - tyA + 1;
    // ---- byte-quad tables of the cells: item = (cell, group of four values); value v -> (tl | tr << 8 | bl << 16 | br << 24)
    const unsigned char *lb = lut + (size_t)b * tiles_x * tiles_y * 256;
    // a wave per cell, a lane per value group: the cell geometry is scalar work
    for (int cell = wv; cell < ncellx * ncelly; cell += 4) {
        const int v4 = lane;
        const int jy = cell / ncellx, jx = cell - jy * ncellx;
        const int c1 = min(max(txA + jx, 0), tiles_x - 1), c2 = min(max(txA + jx + 1, 0), tiles_x - 1);
        const int r1 = min(max(tyA + jy, 0), tiles_y - 1), r2 = min(max(tyA + jy + 1, 0), tiles_y - 1);
        const unsigned A = reinterpret_cast<const unsigned int *>(lb + (unsigned)((r1 * tiles_x + c1) * 256))[v4];
        const unsigned Bq = reinterpret_cast<const unsigned int *>(lb + (unsigned)((r1 * tiles_x + c2) * 256))[v4];
        const unsigned Cq = reinterpret_cast<const unsigned int *>(lb + (unsigned)((r2 * tiles_x + c1) * 256))[v4];
        const unsigned D = reinterpret_cast<const unsigned int *>(lb + (unsigned)((r2 * tiles_x + c2) * 256))[v4];
        // 4 x 4 byte transpose: AB = (A0 B0 A1 B1 | A2 B2 A3 B3), CD alike, then the halves are paired
        const unsigned ab_lo = __builtin_amdgcn_perm(Bq, A, 0x05010400u), ab_hi = __builtin_amdgcn_perm(Bq, A, 0x07030602u);
        const unsigned cd_lo = __builtin_amdgcn_perm(D, Cq, 0x05010400u), cd_hi = __builtin_amdgcn_perm(D, Cq, 0x07030602u);
        uint4 o;
        o.x = __builtin_amdgcn_perm(cd_lo, ab_lo, 0x05040100u); o.y = __builtin_amdgcn_perm(cd_lo, ab_lo, 0x07060302u);
        o.z = __builtin_amdgcn_perm(cd_hi, ab_hi, 0x05040100u); o.w = __builtin_amdgcn_perm(cd_hi, ab_hi, 0x07060302u);
        *reinterpret_cast<uint4 *>(quad + cell * 256 + 4 * v4) = o;
    }
    // ---- row records, lane = staged row (each wave writes and reads only its own copy: no workgroup barrier needed)
    uint4 *rt = rt_all + wv * L0_ROWS;
    {
        const int yr = min(max(reflect101(y0 - 2 + lane, h), 0), h - 1);   // rows past h + 1 feed nothing: clamped garbage
        const float tyf = (float)yr * inv_th - 0.5f;
        const float fy = floorf(tyf);
        const float ya = tyf - fy;
        rt[lane] = make_uint4(__float_as_uint(1.0f - ya), __float_as_uint(ya),
                              (unsigned)(min(max((int)fy - tyA, 0), ncelly - 1) * ncellx) * 1024u, (unsigned)(yr * sstride));
    }
    __builtin_amdgcn_wave_barrier();
    const ov2_level_desc L = pv.lv[0];
    const unsigned char *sb = src + sbstride * b;
    unsigned char *plane = pv.base + L.img_off + L.img_bstride * b;
    const unsigned char *qb = reinterpret_cast<const unsigned char *>(quad);
    if (x0 + L0_TW <= w) l0_rows<true>(sb, w, h, plane, L.istride, pad, inv_tw, txA, ncellx, x0, y0, tile, rt, qb);
    else l0_rows<false>(sb, w, h, plane, L.istride, pad, inv_tw, txA, ncellx, x0, y0, tile, rt, qb);
    if (tid < 128) {   // waves 0, 1: halo dword columns 0 and 33 of every staged row
        const int r = tid >> 1, side = tid & 1, x = x0 - 4 + 4 * 33 * side;
        l0_cols m;
        l0_col_meta(x, w, inv_tw, txA, ncellx, m);
        const uint4 rec = rt[r];
        tile[r][33 * side] = l0_interp(l0_load<false>(sb, rec.w, x, m), m, rec, qb);
    }
    __syncthreads();
    if (x0 <= pad || x0 + L0_TW - 1 >= w - 1 - pad || y0 <= pad || y0 + L0_TH - 1 >= h - 1 - pad)
        l0_border(w, h, plane, L.istride, pad, x0, y0, tile);
    // ---- pyrDown of the staged tile (pyrdown_kernel's second half, l = 0): 16 groups of four outputs x 30 rows
    const ov2_level_desc N = pv.lv[1];
    unsigned char *nplane = pv.base + N.img_off + N.img_bstride * b;
    for (int it = tid; it < (L0_TW / 8) * (L0_TH / 2); it += 256) {
        const int gx = it & 15, ly = it >> 4;
        const int xo = (x0 >> 1) + 4 * gx, yo = (y0 >> 1) + ly;
        if (yo >= N.h || xo >= N.w) continue;
        int acc[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const uint4 q = *reinterpret_cast<const uint4 *>(&tile[2 * ly + j][2 * gx]);
            const unsigned d0 = __builtin_amdgcn_alignbyte(q.y, q.x, 2), d2 = __builtin_amdgcn_alignbyte(q.z, q.y, 2);
            const unsigned wts = 0x04060401u;
            int rr[4];
            rr[0] = (int)__builtin_amdgcn_udot4(d0, wts, (q.y >> 16) & 255u, false);
            rr[1] = (int)__builtin_amdgcn_udot4(q.y, wts, q.z & 255u, false);
            rr[2] = (int)__builtin_amdgcn_udot4(d2, wts, (q.z >> 16) & 255u, false);
            rr[3] = (int)__builtin_amdgcn_udot4(q.z, wts, q.w & 255u, false);
            const int kj = (j == 0 || j == 4) ? 1 : ((j == 2) ? 6 : 4);
#pragma unroll
            for (int o = 0; o < 4; ++o) acc[o] += kj * rr[o];
        }
        const unsigned outp = (unsigned)((acc[0] + 128) >> 8) | ((unsigned)((acc[1] + 128) >> 8) << 8) |
                              ((unsigned)((acc[2] + 128) >> 8) << 16) | ((unsigned)((acc[3] + 128) >> 8) << 24);
        const unsigned no = (unsigned)((yo + pad) * N.istride + OV2_LM + xo);
        const int nv = min(4, N.w - xo);
        if (nv == 4) *reinterpret_cast<unsigned int *>(nplane + no) = outp;
        else for (int o = 0; o < nv; ++o) nplane[no + o] = (unsigned char)(outp >> (8 * o));
        const bool edge = (xo <= pad) || (xo + 3 >= N.w - 1 - pad) || (yo <= pad) || (yo >= N.h - 1 - pad);
        if (edge)
            for (int o = 0; o < nv; ++o) store_reflections(nplane, N.istride, pad, N.w, N.h, xo + o, yo, (unsigned char)(outp >> (8 * o)), false);
    }
}

// ---------------------------------------------------------------------------------------------------
// host side

ov2_status acquire_buf(ov2_ctx *c, int w, int h, int pad, int max_level, int batch, ov2_pyr_buf **out)
{
    {
        // prefer a pooled buffer whose last consumers have already finished: taking the one released a moment ago
        // would chain the new build behind the KLT that still reads it and defeat the two-stream overlap.  A host that
        // runs ahead of the device never finds one, so the pool is a ring: while fewer than pyr_ring buffers of this
        // geometry are pooled with their readers still pending another one is allocated, after that the build takes the
        // one released longest ago (the pool is in release order) and waits for its readers.  A ring of n lets a build
        // start as soon as the tracking call n frames back has ended (ov2_ctx_set_pyr_ring, OV2_PYR_RING).
        std::lock_guard<std::mutex> g(c->mu);
        int pending = -1, npending = 0;
        for (size_t i = 0; i < c->pool.size(); ++i) {
            ov2_pyr_buf *b = c->pool[i];
            if (!(b->w == w && b->h == h && b->pad == pad && b->max_level == max_level && b->batch == batch)) continue;
            if ((!b->has_free_ev || hipEventQuery(b->free_ev) == hipSuccess) &&
                (!b->has_free_ev2 || hipEventQuery(b->free_ev2) == hipSuccess) &&
                (!b->has_free_ev3 || hipEventQuery(b->free_ev3) == hipSuccess)) {
                c->pool.erase(c->pool.begin() + i);
                ++c->pyr_acquires[0];
                *out = b;
                return OV2_OK;
            }
            ++npending;
            if (pending < 0) pending = (int)i;
        }
        if (npending >= c->pyr_ring) {   // the ring is full: reuse rather than grow
            ov2_pyr_buf *b = c->pool[pending];
            c->pool.erase(c->pool.begin() + pending);
            ++c->pyr_acquires[1];
            *out = b;
            return OV2_OK;
        }
    }
    ov2_pyr_buf *b = new ov2_pyr_buf();
    b->w = w; b->h = h; b->pad = pad; b->max_level = max_level; b->batch = batch;
    b->lut = nullptr;
    ov2_pyr_view &v = b->view;
    memset(&v, 0, sizeof(v));
    v.pad = pad;
    v.batch = batch;
    size_t off = 0;
    int cw = w, ch = h, nl = 0;
    for (int l = 0; l <= max_level && l < OV2_MAX_LEVELS; ++l) {
        ov2_level_desc &L = v.lv[l];
        L.w = cw; L.h = ch;
        L.istride = ov2_round_up(OV2_LM + cw + pad, 64);
        L.gstride = ov2_round_up(OV2_LM + cw + pad, 16);
        L.rows = ch + 2 * pad;
        L.img_bstride = ((size_t)L.istride * L.rows + 255) / 256 * 256;
        L.grad_bstride = ((size_t)L.gstride * 4 * L.rows + 255) / 256 * 256;
        L.img_off = off; off += L.img_bstride * batch;
        L.grad_off = off; off += L.grad_bstride * batch;
        nl = l + 1;
        cw = (cw + 1) / 2; ch = (ch + 1) / 2;
        if (cw <= pad || ch <= pad) break;  // buildOpticalFlowPyramid early stop (next level <= winSize)
    }
    v.nlevels = nl;
    b->bytes = off + 4096;
    hipError_t e = hipMalloc((void **)&b->base, b->bytes);
    if (e != hipSuccess) {
        delete b;
        return ov2_set_err(c, OV2_ERR_NOMEM, "pyramid hipMalloc(%zu): %s", off, hipGetErrorString(e));
    }
    e = hipMemsetAsync(b->base, 0, b->bytes, c->stream_pyr);  // gradient padding = 0 for the lifetime of the buffer
    if (e != hipSuccess) {
        (void)hipFree(b->base);
        delete b;
        return ov2_set_err(c, OV2_ERR_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    }
    if (hipEventCreateWithFlags(&b->ready_ev, OV2_ORDER_EVENT_FLAGS) != hipSuccess ||
        hipEventCreateWithFlags(&b->grad_ev, OV2_ORDER_EVENT_FLAGS) != hipSuccess ||
        hipEventCreateWithFlags(&b->free_ev, OV2_ORDER_EVENT_FLAGS) != hipSuccess ||
        hipEventCreateWithFlags(&b->free_ev2, OV2_ORDER_EVENT_FLAGS) != hipSuccess ||
        hipEventCreateWithFlags(&b->free_ev3, OV2_ORDER_EVENT_FLAGS) != hipSuccess) {
        (void)hipFree(b->base);
        delete b;
        return ov2_set_err(c, OV2_ERR_HIP, "hipEventCreate failed");
    }
    b->has_free_ev = false;
    b->has_free_ev2 = false;
    b->has_free_ev3 = false;
    b->kf_seq = 0;
    b->grad_built = false;
    b->build_seq = b->ready_waited_seq = b->grad_waited_seq = 0;
    v.base = b->base;
    {
        std::lock_guard<std::mutex> g(c->mu);
        ++c->pyr_alive;
        ++c->pyr_acquires[2];
    }
    *out = b;
    return OV2_OK;
}

}  // namespace

extern "C" ov2_status ov2_pyramid_build_images(ov2_ctx *c, const ov2_images *im, int win, int max_level,
                                               int use_clahe, float clip, int tiles_x, int tiles_y, ov2_pyr **out)
{
    if (!c || !im || !out) return OV2_ERR_INVALID;
    *out = nullptr;
    if (win < 3 || win > OV2_LM || max_level < 0 || max_level >= OV2_MAX_LEVELS)
        return ov2_set_err(c, OV2_ERR_INVALID, "win=%d (3..%d) max_level=%d (0..%d)", win, OV2_LM, max_level,
                           OV2_MAX_LEVELS - 1);
    if (im->w <= win || im->h <= win) return ov2_set_err(c, OV2_ERR_INVALID, "image smaller than window");
    if (use_clahe && (tiles_x < 1 || tiles_y < 1 || tiles_x > 64 || tiles_y > 64 || tiles_x > im->w || tiles_y > im->h))
        return ov2_set_err(c, OV2_ERR_INVALID, "CLAHE tiles %dx%d", tiles_x, tiles_y);
    OV2_HIP(c, hipSetDevice(c->device));
    ov2_pyr_buf *buf = nullptr;
    ov2_status s = acquire_buf(c, im->w, im->h, win, max_level, im->batch, &buf);
    if (s != OV2_OK) return s;
    const ov2_pyr_view &v = buf->view;
    const int B = im->batch;
    hipStream_t sp = c->stream_pyr;
    // a pooled buffer may still be read by kernels of the main stream (its last consumers): wait for their release mark
    if (buf->has_free_ev) OV2_HIP(c, hipStreamWaitEvent(sp, buf->free_ev, 0));
    if (buf->has_free_ev2) {   // readers another context enqueued on its own stream (ov2_pyr_release_from)
        OV2_HIP(c, hipStreamWaitEvent(sp, buf->free_ev2, 0));
        buf->has_free_ev2 = false;
    }
    if (buf->has_free_ev3) {   // a detector chain that read it from the keyframe side stream beside the main stream (ov2_pyr_release)
        OV2_HIP(c, hipStreamWaitEvent(sp, buf->free_ev3, 0));
        buf->has_free_ev3 = false;
        c->stream.kfj[OV2_KFJ_PYR].fetch_add(1, std::memory_order_relaxed);
    }
    buf->kf_seq = 0;

    float inv_tw = 0.f, inv_th = 0.f;
    if (use_clahe) {
        if (!buf->lut) {
            hipError_t e = hipMalloc((void **)&buf->lut, (size_t)B * 64 * 64 * 256);
            if (e != hipSuccess) {
                std::lock_guard<std::mutex> g(c->mu);
                c->pool.push_back(buf);
                return ov2_set_err(c, OV2_ERR_NOMEM, "CLAHE LUT hipMalloc");
            }
        }
        int ew = im->w, eh = im->h;
        if (im->w % tiles_x != 0 || im->h % tiles_y != 0) {  // CLAHE_Impl::apply: extend right/bottom
            ew = im->w + (tiles_x - im->w % tiles_x);
            eh = im->h + (tiles_y - im->h % tiles_y);
        }
        const int tw = ew / tiles_x, th = eh / tiles_y;
        const int total = tw * th;
        const float lut_scale = 255.0f / (float)total;
        int clip_limit = 0;
        if ((double)clip > 0.0) {
            clip_limit = (int)((double)clip * total / 256);
            if (clip_limit < 1) clip_limit = 1;
        }
        inv_tw = 1.0f / (float)tw;
        inv_th = 1.0f / (float)th;
        OV2_LAUNCH_ON(c, OV2_K_CLAHE_LUT, sp, clahe_lut_wave_kernel, dim3((tiles_x * tiles_y + 3) / 4, B), dim3(256), 0, sp, im->base, im->w,
                           im->h, im->stride, im->bstride, tiles_x, tiles_y, tw, th, clip_limit, lut_scale, buf->lut, c->wave_prio);
    }
    int ncx_max = 0, ncy_max = 0;
    size_t l0_lds = 0;
    if (use_clahe) {
        // upper bound of the LUT window of a 64 x 16 px tile; tw/th = 1 / inv
        const float tw = 1.0f / inv_tw, th = 1.0f / inv_th;
        ncx_max = (int)(64.0f / tw) + 3;
        ncy_max = (int)(64.0f / th) + 3;
        l0_lds = (size_t)ncx_max * ncy_max * 256;
    }
    // fused level 0 + first pyrDown: LDS = the staged tile + one 1-KB quad table per interpolation cell it can touch
    int first_down = 0;
    size_t fused_lds = 0;
    if (use_clahe && v.nlevels >= 2) {
        const float tw = 1.0f / inv_tw, th = 1.0f / inv_th;
        const int cells = ((int)((float)(L0_TW + 16) / tw) + 2) * ((int)((float)(L0_TH + 4) / th) + 2);
        fused_lds = ((size_t)L0_ROWS * L0_DW + 4 * L0_RT_DW + (size_t)cells * 256) * 4;
    }
    if (use_clahe && v.nlevels >= 2 && fused_lds <= 64 * 1024 && im->w >= 8 && im->h >= 8) {
        OV2_LAUNCH_ON(c, OV2_K_LEVEL0, sp, level0_clahe_pyrdown_kernel, dim3((im->w + L0_TW - 1) / L0_TW, (im->h + L0_TH - 1) / L0_TH, B),
                      dim3(256), fused_lds, sp, im->base, im->w, im->h, im->stride, im->bstride, buf->lut, tiles_x, tiles_y, inv_tw,
                      inv_th, v, c->wave_prio);
        first_down = 1;
    } else if (use_clahe && l0_lds <= 48 * 1024)
        OV2_LAUNCH_ON(c, OV2_K_LEVEL0, sp, level0_clahe_tiled_kernel, dim3((im->w + 63) / 64, (im->h + 63) / 64, B), dim3(256), l0_lds,
                   sp, im->base, im->w, im->h, im->stride, im->bstride, buf->lut, tiles_x, tiles_y, inv_tw, inv_th,
                   ncx_max, v, c->wave_prio);
    else {
        OV2_LAUNCH_ON(c, OV2_K_LEVEL0, sp, level0_kernel, dim3((im->w + 255) / 256, im->h, B), dim3(64), 0, sp, im->base, im->w,
                      im->h, im->stride, im->bstride, use_clahe, buf->lut, tiles_x, tiles_y, inv_tw, inv_th, v, c->wave_prio);
    }
    // pyrDown chain only: the gradient planes are written when a consumer asks for them (ov2_pyr_need_grad)
    // a new build: whatever the main stream waited for in this buffer was an earlier one
    { std::lock_guard<std::mutex> g(c->mu); buf->grad_built = false; ++buf->build_seq; }
    // two levels per launch while two are left, then one
    int l = first_down;
    for (; l + 2 < v.nlevels; l += 2) {
        const ov2_level_desc &M = v.lv[l + 2];
        OV2_LAUNCH_ON(c, OV2_K_LEVEL, sp, pyrdown2_kernel, dim3((M.w + P2_TW - 1) / P2_TW, (M.h + P2_TH - 1) / P2_TH, B), dim3(256), 0,
                      sp, v, l, c->wave_prio);
    }
    for (; l + 1 < v.nlevels; ++l) {
        const ov2_level_desc &L = v.lv[l];
        OV2_LAUNCH_ON(c, OV2_K_LEVEL, sp, pyrdown_kernel, dim3((L.w + PD_TW - 1) / PD_TW, (L.h + PD_TH - 1) / PD_TH, B), dim3(256), 0, sp,
                      v, l, c->wave_prio);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        std::lock_guard<std::mutex> g(c->mu);
        c->pool.push_back(buf);
        return ov2_set_err(c, OV2_ERR_HIP, "pyramid launch: %s", hipGetErrorString(e));
    }
    OV2_HIP(c, hipEventRecord(buf->ready_ev, sp));
    ov2_pyr *p = new ov2_pyr();
    p->refs.store(1);
    p->ctx = c;
    p->buf = buf;
    *out = p;
    return OV2_OK;
}

extern "C" ov2_status ov2_pyramid_build(ov2_ctx *c, const uint8_t *img, int w, int h, int stride, int win,
                                        int max_level, int use_clahe, float clip, int tiles_x, int tiles_y,
                                        ov2_pyr **out)
{
    if (!c || !img || !out || w <= 0 || h <= 0 || stride < w) return OV2_ERR_INVALID;
    if (c->tmp_img && (c->tmp_img->w != w || c->tmp_img->h != h)) {
        OV2_HIP(c, hipStreamSynchronize(c->stream));
        ov2_images_destroy(c->tmp_img);
        c->tmp_img = nullptr;
    }
    if (!c->tmp_img) {
        ov2_status s = ov2_images_create(c, 1, w, h, &c->tmp_img);
        if (s != OV2_OK) return s;
    }
    ov2_status s = ov2_images_upload(c, c->tmp_img, 0, img, stride);
    if (s != OV2_OK) return s;
    s = ov2_pyramid_build_images(c, c->tmp_img, win, max_level, use_clahe, clip, tiles_x, tiles_y, out);
    if (s != OV2_OK) return s;
    OV2_HIP(c, hipStreamSynchronize(c->stream_pyr));  // the staging image may be overwritten by the next call
    return OV2_OK;
}

extern "C" void ov2_pyr_retain(ov2_pyr *p)
{
    if (p) p->refs.fetch_add(1);
}

extern "C" void ov2_pyr_release(ov2_pyr *p)
{
    if (!p) return;
    if (p->refs.fetch_sub(1) == 1) {
        // stream-ordered reuse: later builds on the same ctx stream run after every kernel that reads this buffer
        // when those readers were enqueued on the same ctx.  Cross-ctx readers must synchronise before release.
        // every consumer of this pyramid was enqueued on the main stream before this release: mark that point
        if (hipEventRecord(p->buf->free_ev, p->ctx->stream.h) == hipSuccess) p->buf->has_free_ev = true;
        // ... except a detector chain that reads it on the keyframe side stream while the main stream is not behind that
        // chain: everything the side stream holds is marked too (a mark that cannot be recorded is waited out here)
        if (p->buf->kf_seq > p->ctx->stream.joined_seq.load(std::memory_order_acquire)) {
            if (hipEventRecord(p->buf->free_ev3, p->ctx->stream_kf) == hipSuccess) p->buf->has_free_ev3 = true;
            else (void)hipStreamSynchronize(p->ctx->stream_kf);
        }
        std::lock_guard<std::mutex> g(p->ctx->mu);
        p->ctx->pool.push_back(p->buf);
        delete p;
    }
}

// A consumer on ANOTHER context (the reference's mapper thread works on the keyframe's pyramid while the front-end
// moves on, src/mapper.cpp:76-97) enqueued its readers on `user`'s main stream: mark that point on the buffer, so
// the next build into it waits for them, then drop the reference.  One foreign consumer stream per pyramid.
extern "C" void ov2_pyr_release_from(ov2_ctx *user, ov2_pyr *p)
{
    if (!p) return;
    if (user && user != p->ctx) {
        (void)hipSetDevice(user->device);
        std::lock_guard<std::mutex> g(p->ctx->mu);
        if (hipEventRecord(p->buf->free_ev2, user->stream.h) == hipSuccess) p->buf->has_free_ev2 = true;
    }
    ov2_pyr_release(p);
}

extern "C" int ov2_pyr_batch(const ov2_pyr *p) { return p ? p->buf->batch : 0; }
extern "C" int ov2_pyr_nlevels(const ov2_pyr *p) { return p ? p->buf->view.nlevels : 0; }

extern "C" ov2_status ov2_pyr_level_size(const ov2_pyr *p, int level, int *w, int *h, int *pad)
{
    if (!p || level < 0 || level >= p->buf->view.nlevels) return OV2_ERR_INVALID;
    if (w) *w = p->buf->view.lv[level].w;
    if (h) *h = p->buf->view.lv[level].h;
    if (pad) *pad = p->buf->view.pad;
    return OV2_OK;
}

extern "C" ov2_status ov2_pyr_download_level(ov2_ctx *c, const ov2_pyr *p, int b, int level, uint8_t *img,
                                             int16_t *grad)
{
    if (!c || !p || b < 0 || b >= p->buf->batch || level < 0 || level >= p->buf->view.nlevels) return OV2_ERR_INVALID;
    const ov2_pyr_view &v = p->buf->view;
    const ov2_level_desc &L = v.lv[level];
    const int pw = L.w + 2 * v.pad, ph = L.h + 2 * v.pad;
    const int x_off = OV2_LM - v.pad;
    if (grad) {
        const ov2_status gs = ov2_pyr_need_grad(c, p);
        if (gs != OV2_OK) return gs;
    }
    OV2_HIP(c, hipStreamSynchronize(c->stream_pyr));
    OV2_HIP(c, hipStreamSynchronize(c->stream));
    if (img)
        OV2_HIP(c, hipMemcpy2D(img, pw, v.base + L.img_off + L.img_bstride * b + x_off, L.istride, pw, ph,
                               hipMemcpyDeviceToHost));
    if (grad)
        OV2_HIP(c, hipMemcpy2D(grad, (size_t)pw * 4, v.base + L.grad_off + L.grad_bstride * b + (size_t)x_off * 4,
                               (size_t)L.gstride * 4, (size_t)pw * 4, ph, hipMemcpyDeviceToHost));
    return OV2_OK;
}

namespace {

// Puts c's main stream behind `ev` (ready_ev or grad_ev of p's buffer) unless it provably is already.  Call with the OWNING
// context's mutex held.  The owner's main stream needs one wait per build: `*waited_seq` names the build it has waited
// for, and every later call finds the stream behind that point already (the second call of a frame loop that tracks
// t - 1 -> t, then t -> t + 1; the detector behind the stereo call of a keyframe).  An event that has completed orders
// nothing either, so a host that does not run ahead of the device issues no packet at all.  A consumer on another
// context has a stream of its own and no record here: it always waits.  The keyframe side stream needs no wait of its
// own, its chain starts from an event recorded on the main stream behind this point (detect.hip).
hipError_t wait_once(ov2_ctx *c, const ov2_pyr *p, hipEvent_t ev, unsigned long long *waited_seq)
{
    const ov2_pyr_buf *buf = p->buf;
    const bool own = c == p->ctx;
    if (own && *waited_seq == buf->build_seq) {
        c->pyr_waits[1].fetch_add(1, std::memory_order_relaxed);
        return hipSuccess;
    }
    if (own && hipEventQuery(ev) == hipSuccess) {
        *waited_seq = buf->build_seq;
        c->pyr_waits[1].fetch_add(1, std::memory_order_relaxed);
        c->pyr_waits[2].fetch_add(1, std::memory_order_relaxed);
        return hipSuccess;
    }
    const hipError_t err = hipStreamWaitEvent(c->stream.h, ev, 0);   // ordering only: not a use of the main stream (ov2_main_stream)
    if (err == hipSuccess) {
        if (own) *waited_seq = buf->build_seq;
        c->pyr_waits[0].fetch_add(1, std::memory_order_relaxed);
    }
    return err;
}

}  // namespace

// Scharr planes of every level, written once per pyramid by the first consumer that needs them (the 8 / 16-lane KLT
// kernels, ov2_pyr_download_level) on ITS main stream, behind the build; later consumers wait for that point.
ov2_status ov2_pyr_need_grad(ov2_ctx *c, const ov2_pyr *p)
{
    if (!c || !p) return OV2_ERR_INVALID;
    if (c->device != p->ctx->device) return ov2_set_err(c, OV2_ERR_INVALID, "pyramid of device %d used on device %d", p->ctx->device, c->device);
    ov2_pyr_buf *buf = p->buf;
    // The HIP calls run under the owning context's mutex (two consumer contexts must not both write the planes), so their
    // failures are collected and reported AFTER the guard is gone: ov2_set_err locks the same mutex when c == p->ctx.
    hipError_t err = hipSuccess;
    const char *what = "";
    {
        std::lock_guard<std::mutex> g(p->ctx->mu);
        if (buf->grad_built) {
            err = wait_once(c, p, buf->grad_ev, &buf->grad_waited_seq); what = "hipStreamWaitEvent(grad_ev)";
            // the planes were written behind the build: a stream behind them is behind the build as well
            if (err == hipSuccess && c == p->ctx) buf->ready_waited_seq = buf->build_seq;
        } else if ((err = wait_once(c, p, buf->ready_ev, &buf->ready_waited_seq)) != hipSuccess) {
            what = "hipStreamWaitEvent(ready_ev)";
        } else {
            const ov2_pyr_view &v = buf->view;
            for (int l = 0; l < v.nlevels; ++l) {
                const ov2_level_desc &L = v.lv[l];
                OV2_LAUNCH(c, OV2_K_LEVEL, level_kernel, dim3((L.w + TILE_W - 1) / TILE_W, (L.h + TILE_H - 1) / TILE_H, buf->batch), dim3(256), 0,
                           c->stream, v, l, 0, 1, c->wave_prio);
            }
            if ((err = hipGetLastError()) != hipSuccess) what = "level_kernel launch";
            else if ((err = hipEventRecord(buf->grad_ev, c->stream)) != hipSuccess) what = "hipEventRecord(grad_ev)";
            else {
                buf->grad_built = true;
                if (c == p->ctx) buf->grad_waited_seq = buf->build_seq;   // written on this very stream: ordered without an event
            }
        }
    }
    if (err != hipSuccess) return ov2_set_err(c, OV2_ERR_HIP, "%s failed: %s", what, hipGetErrorString(err));
    return OV2_OK;
}

ov2_status ov2_pyr_wait_ready(ov2_ctx *c, const ov2_pyr *p)
{
    if (!c || !p) return OV2_ERR_INVALID;
    // the pool's events carry no system-scope fence (OV2_ORDER_EVENT_FLAGS) and the kernels read the buffer directly: a
    // consumer context must sit on the device the pyramid was built on
    if (c->device != p->ctx->device) return ov2_set_err(c, OV2_ERR_INVALID, "pyramid of device %d used on device %d", p->ctx->device, c->device);
    hipError_t err;
    {
        std::lock_guard<std::mutex> g(p->ctx->mu);
        err = wait_once(c, p, p->buf->ready_ev, &p->buf->ready_waited_seq);
    }
    if (err != hipSuccess) return ov2_set_err(c, OV2_ERR_HIP, "hipStreamWaitEvent(ready_ev) failed: %s", hipGetErrorString(err));
    return OV2_OK;
}
