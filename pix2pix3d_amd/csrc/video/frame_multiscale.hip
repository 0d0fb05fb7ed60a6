// Multi-scale frame quality for gfx950 (p3d_video.h, "multi-scale frame quality"; pix2pix3d_amd/multiscale.py): the 2 x 2
// pyramid of a clip and, per level, the sums behind MS-SSIM in the integers of the header's SSIM.  The rules are the header's; the torch
// formulation of multiscale.py produces the same bytes.
//
// p3d_frame_halve          256 threads: 64 lanes along a row by 4 waves, a wave every fourth of the tile's 16 output rows, frames on grid.z (strided
//                          past 65535).  A lane owns G = 4 output bytes (12 at three bytes a pixel, so that a lane begins on a pixel AND a dword):
//                          2 G consecutive source bytes of two rows — dword loads and dword stores where the three rows start on a dword, bytes
//                          elsewhere and at the row's tail.
// p3d_frame_msssim_level   a work-group owns a tile of 32 x 16 PIXELS of one frame, all channels: the windows that BEGIN in the tile and the
//                          16 x 8 samples of the next level under it.  The 42 x 26 samples of both clips that lie inside the frame go to LDS once,
//                          as dwords where the global address allows (the LDS copy keeps the address's low two bits, so that an aligned dword stays
//                          aligned); the next level of both clips is written from them straight away, 4 bytes a lane; then per channel the
//                          passes of ssim_window.h, which p3d_video_ssim runs too — the horizontal one into LDS, a barrier, the vertical one a
//                          lane a window, two windows a lane.  q and cs meet in wave reductions and the
//                          work-group issues ONE atomic per slot and channel.  A tile at the right or bottom edge without a window of its own
//                          skips the passes (the condition is the same for the whole work-group) and still writes its samples of the next level.
#include "../p3d_common.h"
#include "clip_checks.h"
#include "p3d_video.h"
#include "ssim_window.h"

namespace {

using namespace p3d;
using namespace p3d::ssim;                                                      // kThreads, kWaves, the window's tile: one work-group shape for both kernels

constexpr int kMaxGridZ = 65535;

// ---- the pyramid step -------------------------------------------------------------------------------------------------------------------------
constexpr int kHalveTileH = 16, kHalveRowsPerWave = kHalveTileH / kWaves;

struct Halve { const uint8_t* src; int64_t sfp, srp; uint8_t* dst; int64_t dfp, drp; int frames, nh, nw; };

__device__ __forceinline__ int byte_of(const uint32_t* words, int i) { return (int)((words[i >> 2] >> (8 * (i & 3))) & 0xffu); }

template <int BPP>
__global__ void __launch_bounds__(kThreads) halve_kernel(const Halve g)
{
    constexpr int G = BPP == 3 ? 12 : 4;                                        // output bytes of a lane: whole pixels and whole dwords
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t out_row = (int64_t)g.nw * BPP;
    const int64_t ob = ((int64_t)blockIdx.x * kWave + lane) * G;                // the lane's first output byte of a row
    if (ob >= out_row) return;
    const int n = out_row - ob < G ? (int)(out_row - ob) : G;                   // a multiple of BPP
    for (int f = blockIdx.z; f < g.frames; f += gridDim.z) {
        for (int j = 0; j < kHalveRowsPerWave; ++j) {
            const int y = blockIdx.y * kHalveTileH + wave + j * kWaves;
            if (y >= g.nh) break;
            const uint8_t* const r0 = g.src + (int64_t)f * g.sfp + (int64_t)(2 * y) * g.srp + 2 * ob;      // 2 n bytes of rows 2 y and 2 y + 1: inside
            const uint8_t* const r1 = r0 + g.srp;                                                          // the rows, as 2 nw <= w
            uint8_t* const d = g.dst + (int64_t)f * g.dfp + (int64_t)y * g.drp + ob;
            if (n == G && ((((uintptr_t)r0) | ((uintptr_t)r1) | ((uintptr_t)d)) & 3u) == 0) {
                uint32_t s0[G / 2], s1[G / 2], o[G / 4];
#pragma unroll
                for (int i = 0; i < G / 2; ++i) {
                    s0[i] = reinterpret_cast<const uint32_t*>(r0)[i];
                    s1[i] = reinterpret_cast<const uint32_t*>(r1)[i];
                }
#pragma unroll
                for (int i = 0; i < G / 4; ++i) o[i] = 0;
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    const int i0 = 2 * (k / BPP) * BPP + k % BPP, i1 = i0 + BPP;
                    const int v = (byte_of(s0, i0) + byte_of(s0, i1) + byte_of(s1, i0) + byte_of(s1, i1) + 2) >> 2;
                    o[k >> 2] |= (uint32_t)v << (8 * (k & 3));
                }
#pragma unroll
                for (int i = 0; i < G / 4; ++i) reinterpret_cast<uint32_t*>(d)[i] = o[i];
            } else {
                for (int k = 0; k < n; ++k) {
                    const int i0 = 2 * (k / BPP) * BPP + k % BPP, i1 = i0 + BPP;
                    d[k] = (uint8_t)(((int)r0[i0] + (int)r0[i1] + (int)r1[i0] + (int)r1[i1] + 2) >> 2);
                }
            }
        }
    }
}

// ---- one level ----------------------------------------------------------------------------------------------------------------------------
constexpr int kRowWords = (kInW * 4 + 3 + 3) / 4;                               // dwords of a staged row: 168 bytes behind a shift of up to 3; 43, odd
static_assert(kTileW == P3D_MSSSIM_TILE_W && kTileH == P3D_MSSSIM_TILE_H, "the pixel tile is the window tile of ssim_window.h");
static_assert(kTileW % 2 == 0 && kTileH % 2 == 0, "no 2 x 2 block of the next level straddles two tiles");

struct Level {
    const uint8_t* a; int64_t a_frame_pitch, a_row_pitch;
    const uint8_t* b; int64_t b_frame_pitch, b_row_pitch;
    int H, W;
    int per_frame, tiles_x;                                                     // pixel tiles of a frame, and of a row of them
    unsigned long long* sums; int64_t sums_pitch;
    uint8_t* next_a; uint8_t* next_b;
};

// Dword d of a staged row: the row's bytes [0, span) stand at LDS bytes [shift, shift + span), shift = the global address's low two bits.
__device__ __forceinline__ uint32_t staged_word(const uint8_t* row, int shift, int d, int span)
{
    const int b0 = d * 4 - shift;                                               // the row's byte that is byte 0 of this dword
    uint32_t v = 0;
    if (b0 >= 0 && b0 + 4 <= span) {
        v = *reinterpret_cast<const uint32_t*>(row + b0);                       // (row + b0 = row - shift + 4 d: on a dword)
    } else {
        for (int k = 0; k < 4; ++k)
            if (b0 + k >= 0 && b0 + k < span) v |= (uint32_t)row[b0 + k] << (8 * k);
    }
    return v;
}

template <int BPP>
__global__ void __launch_bounds__(kThreads) msssim_level_kernel(const Level p)
{
    __shared__ uint32_t ta[kInH * kRowWords], tb[kInH * kRowWords];             // 2 x 4472 bytes
    __shared__ RowSums hb;
    __shared__ long long part[2][kWaves];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & (kWave - 1);
    const int f = blockIdx.x / (unsigned)p.per_frame;
    const int tile = blockIdx.x - f * p.per_frame;
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const int x0 = tx * kTileW, y0 = ty * kTileH;                               // even; x0 < W, y0 < H
    const int oh = p.H - kHalo, ow = p.W - kHalo;
    const int tw = min(kTileW, ow - x0), th = min(kTileH, oh - y0);             // the windows that begin in the tile; <= 0: none
    const int rows_in = min(kInH, p.H - y0), cols_in = min(kInW, p.W - x0);     // what of the 42 x 26 samples lies inside the frame
    const int span = cols_in * BPP;                                             // <= 168
    const uint8_t* const fa = p.a + f * p.a_frame_pitch + y0 * p.a_row_pitch + (int64_t)x0 * BPP;
    const uint8_t* const fb = p.b + f * p.b_frame_pitch + y0 * p.b_row_pitch + (int64_t)x0 * BPP;
    const int a_base = (int)((uintptr_t)fa & 3u), a_step = (int)(p.a_row_pitch & 3), b_base = (int)((uintptr_t)fb & 3u), b_step = (int)(p.b_row_pitch & 3);
    for (int i = tid; i < rows_in * kRowWords; i += kThreads) {
        const int r = i / kRowWords, d = i - r * kRowWords;
        ta[i] = staged_word(fa + r * p.a_row_pitch, (a_base + r * a_step) & 3, d, span);
        tb[i] = staged_word(fb + r * p.b_row_pitch, (b_base + r * b_step) & 3, d, span);
    }
    __syncthreads();
    const uint8_t* const sa = reinterpret_cast<const uint8_t*>(ta);
    const uint8_t* const sb = reinterpret_cast<const uint8_t*>(tb);

    if (p.next_a) {                                                             // the next level of both clips: 16 x 8 pixels under the tile, 4 bytes a lane
        constexpr int kRowItems = kTileW / 2 * BPP / 4, kItems = kRowItems * (kTileH / 2);      // 4 BPP dwords a row, 32 BPP <= 128 a clip
        const int nh = p.H >> 1, nw = p.W >> 1, nx0 = x0 >> 1, ny0 = y0 >> 1;
        const int valid = min(kTileW / 2, nw - nx0) * BPP;                      // bytes of a tile row inside the next level; <= 0: none
        for (int i = tid; i < 2 * kItems; i += kThreads) {
            const int second = i >= kItems, j = i - second * kItems;
            const int row = j / kRowItems, at = (j - row * kRowItems) * 4;      // output row of the tile, first byte of it
            const int ny = ny0 + row;
            if (ny >= nh || at >= valid) continue;
            const uint8_t* const s = second ? sb : sa;
            const int base = second ? b_base : a_base, step = second ? b_step : a_step;
            const uint8_t* const r0 = s + (2 * row) * (kRowWords * 4) + ((base + 2 * row * step) & 3);
            const uint8_t* const r1 = s + (2 * row + 1) * (kRowWords * 4) + ((base + (2 * row + 1) * step) & 3);
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {                                       // (a byte past `valid` reads LDS inside the arrays and is never stored)
                const int px = (at + k) / BPP, c = (at + k) - px * BPP;
                const int i0 = 2 * px * BPP + c, i1 = i0 + BPP;
                v |= (uint32_t)(((int)r0[i0] + (int)r0[i1] + (int)r1[i0] + (int)r1[i1] + 2) >> 2) << (8 * k);
            }
            uint8_t* const dst = (second ? p.next_b : p.next_a) + (((int64_t)f * nh + ny) * nw + nx0) * BPP + at;
            if (at + 4 <= valid && ((uintptr_t)dst & 3u) == 0) {
                *reinterpret_cast<uint32_t*>(dst) = v;
            } else {
                for (int k = 0; k < 4; ++k)
                    if (at + k < valid) dst[k] = (uint8_t)(v >> (8 * k));
            }
        }
    }
    if (tw <= 0 || th <= 0) return;                                             // the whole work-group: no barrier follows for anyone

    const int ih = th + kHalo;                                                  // <= rows_in
    for (int c = 0; c < BPP; ++c) {
        for (int i = tid; i < ih * kTileW; i += kThreads) {                     // the horizontal pass
            const int r = i >> 5, x = i & (kTileW - 1);
            if (x < tw) {
                const uint8_t* const ra = sa + r * (kRowWords * 4) + ((a_base + r * a_step) & 3) + x * BPP + c;
                const uint8_t* const rb = sb + r * (kRowWords * 4) + ((b_base + r * b_step) & 3) + x * BPP + c;
                int s[5] = {};
#pragma unroll
                for (int k = 0; k < kTaps; ++k) row_tap(s, ra[k * BPP], rb[k * BPP], k);
                put_row_sums(hb, r, x, s);
            }
        }
        __syncthreads();
        long long mine_q = 0, mine_cs = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {                                           // the vertical pass: window (x, y) of the tile
            const int o = tid + j * kThreads, y = o >> 5, x = o & (kTileW - 1);
            if (y < th && x < tw) {
                Moments m{0, 0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < kTaps; ++k) column_tap(m, hb, y, x, k);
                double cs;
                const double q = window_values<true>(m, &cs);
                mine_q += contribution(q);
                mine_cs += contribution(cs);
            }
        }
        mine_q = wave_sum(mine_q);
        mine_cs = wave_sum(mine_cs);
        if (lane == 0) { part[0][wave] = mine_q; part[1][wave] = mine_cs; }
        __syncthreads();                                                        // (also: every read of hb came before the next channel's writes)
        if (tid < 3) {                                                          // ONE atomic per slot
            long long total = (long long)tw * th;
            if (tid < 2) {
                total = 0;
#pragma unroll
                for (int w = 0; w < kWaves; ++w) total += part[tid][w];
            }
            atomicAdd(p.sums + ((int64_t)f * BPP + c) * p.sums_pitch + tid, (unsigned long long)total);
        }
        __syncthreads();                                                        // part is free again
    }
}

} // namespace

extern "C" int p3d_frame_halve(const uint8_t* src, int64_t src_frame_pitch, int64_t src_row_pitch, int32_t frames, int32_t h, int32_t w, int32_t bpp,
                               uint8_t* dst, int64_t dst_frame_pitch, int64_t dst_row_pitch, p3d_stream_t stream)
{
    using namespace p3d;
    int64_t pixels = 0;
    if (int code = check_clip_sizes("frame_halve", frames, h, w, bpp, &pixels)) return code;
    const int nh = h / 2, nw = w / 2;
    if ((int64_t)frames * nh * nw == 0) return P3D_OK;
    P3D_REQUIRE(src && dst, "frame_halve: a clip pointer is null");
    const int64_t src_row = (int64_t)w * bpp, dst_row = (int64_t)nw * bpp;
    P3D_REQUIRE(src_row_pitch >= src_row && dst_row_pitch >= dst_row, "frame_halve: a row pitch is below its row (%lld < %lld or %lld < %lld)",
                (long long)src_row_pitch, (long long)src_row, (long long)dst_row_pitch, (long long)dst_row);
    const int64_t src_frame = (int64_t)(h - 1) * src_row_pitch + src_row, dst_frame = (int64_t)(nh - 1) * dst_row_pitch + dst_row;
    P3D_REQUIRE(src_frame_pitch >= 0 && (frames == 1 || dst_frame_pitch >= dst_frame),
                "frame_halve: the source's frame pitch must not be negative and the destination's frames must not overlap");
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)((int64_t)(frames - 1) * src_frame_pitch + src_frame);
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)((int64_t)(frames - 1) * (frames == 1 ? 0 : dst_frame_pitch) + dst_frame);
    P3D_REQUIRE(d1 <= s0 || s1 <= d0, "frame_halve writes out of place: the destination's bytes meet the source's");
    const Halve g{src, src_frame_pitch, src_row_pitch, dst, dst_frame_pitch, dst_row_pitch, frames, nh, nw};
    const int64_t lanes = (dst_row + (bpp == 3 ? 12 : 4) - 1) / (bpp == 3 ? 12 : 4);
    const dim3 grid((unsigned)((lanes + kWave - 1) / kWave), (unsigned)((nh + kHalveTileH - 1) / kHalveTileH), (unsigned)(frames < kMaxGridZ ? frames : kMaxGridZ));
    switch (bpp) {
    case 1: hipLaunchKernelGGL(halve_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, g); break;
    case 2: hipLaunchKernelGGL(halve_kernel<2>, grid, dim3(kThreads), 0, (hipStream_t)stream, g); break;
    case 3: hipLaunchKernelGGL(halve_kernel<3>, grid, dim3(kThreads), 0, (hipStream_t)stream, g); break;
    default: hipLaunchKernelGGL(halve_kernel<4>, grid, dim3(kThreads), 0, (hipStream_t)stream, g); break;
    }
    count_launch(FAM_AUX);
    return check_launch("frame_halve");
}

extern "C" int p3d_frame_msssim_level(const uint8_t* a, int64_t a_frame_pitch, int64_t a_row_pitch, const uint8_t* b, int64_t b_frame_pitch,
                                      int64_t b_row_pitch, int32_t frames, int32_t h, int32_t w, int32_t bpp, int64_t* sums, int64_t sums_pitch,
                                      uint8_t* next_a, uint8_t* next_b, p3d_stream_t stream)
{
    using namespace p3d;
    int64_t pixels = 0;
    const int rc = check_pair("frame_msssim_level", a, a_frame_pitch, a_row_pitch, b, b_frame_pitch, b_row_pitch, frames, h, w, bpp, sums, &pixels);
    if (rc != P3D_OK || pixels == 0) return rc;
    P3D_REQUIRE(h >= kTaps && w >= kTaps, "frame_msssim_level: a level of %d x %d has no %d x %d window", w, h, kTaps, kTaps);
    P3D_REQUIRE(sums_pitch >= 3, "frame_msssim_level: sums_pitch must be at least 3 (got %lld)", (long long)sums_pitch);
    P3D_REQUIRE((next_a == nullptr) == (next_b == nullptr), "frame_msssim_level: next_a and next_b are both given or both null");
    P3D_REQUIRE(next_a == nullptr || next_a != next_b, "frame_msssim_level: next_a and next_b must be two buffers");
    Level p{a, a_frame_pitch, a_row_pitch, b, b_frame_pitch, b_row_pitch, h, w, 0, 0, (unsigned long long*)sums, sums_pitch, next_a, next_b};
    p.tiles_x = ceil_div(w, kTileW);
    p.per_frame = p.tiles_x * ceil_div(h, kTileH);
    const dim3 grid((unsigned)((int64_t)frames * p.per_frame));                 // < 2^31, as the pixels are
    switch (bpp) {
    case 1: hipLaunchKernelGGL(msssim_level_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, p); break;
    case 2: hipLaunchKernelGGL(msssim_level_kernel<2>, grid, dim3(kThreads), 0, (hipStream_t)stream, p); break;
    case 3: hipLaunchKernelGGL(msssim_level_kernel<3>, grid, dim3(kThreads), 0, (hipStream_t)stream, p); break;
    default: hipLaunchKernelGGL(msssim_level_kernel<4>, grid, dim3(kThreads), 0, (hipStream_t)stream, p); break;
    }
    count_launch(FAM_AUX);
    return check_launch("frame_msssim_level");
}
