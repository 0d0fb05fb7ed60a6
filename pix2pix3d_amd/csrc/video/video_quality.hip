// Frame quality where the frames are (p3d_video.h; pix2pix3d_amd/quality.py): the error sums behind MAE, MSE and PSNR, and SSIM in
// the header's integers.  Both kernels ADD to the caller's int64 counters: integer sums, so neither the order of the work-groups nor that of the calls shows.
//
// p3d_video_error_sums  a work-group of four waves owns kErrPixels consecutive pixels of one frame, a lane every 256th of them, all channels of a pixel in
//                       its own registers.  16 values leave a lane; a wave reduction, 4 x 16 words of LDS, and the first 4 bpp lanes issue ONE atomic each.
// p3d_video_ssim        a work-group owns a tile of 32 x 16 windows of one frame, all channels.  The 42 x 26 samples under it, of both clips, go to LDS once
//                       (as bytes, channels interleaved as in memory); then per channel the passes of ssim_window.h — the horizontal one into LDS, a
//                       barrier, the vertical one a lane a window, two windows a lane.  The contributions meet in a wave reduction and ONE atomic a
//                       channel and work-group.
#include "../p3d_common.h"
#include "clip_checks.h"
#include "p3d_video.h"
#include "ssim_window.h"

namespace {

using namespace p3d;
using namespace p3d::ssim;                                                      // kThreads, kWaves, the tile and wave_sum: one work-group shape for both kernels

constexpr int kErrPixels = kThreads * 16;                                       // of a work-group of the error sums

struct PairArgs {
    const uint8_t* a; int64_t a_frame_pitch, a_row_pitch;
    const uint8_t* b; int64_t b_frame_pitch, b_row_pitch;
    int H, W, bpp;
    int per_frame;                                                              // work-groups of a frame
    int tiles_x;                                                                // SSIM only
    unsigned long long* sums;
    float* map;
};

__device__ __forceinline__ long long wave_max(long long v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) { const long long t = __shfl_down(v, d); v = t > v ? t : v; }
    return v;
}

__global__ void __launch_bounds__(kThreads) error_sums_kernel(const PairArgs p)
{
    __shared__ long long part[kWaves][16];
    const int f = blockIdx.x / (unsigned)p.per_frame;
    const int chunk = blockIdx.x - f * p.per_frame;
    const int pixels = p.H * p.W;                                               // < 2^31
    const int first = chunk * kErrPixels, last = min(first + kErrPixels, pixels);
    const uint8_t* const fa = p.a + f * p.a_frame_pitch;
    const uint8_t* const fb = p.b + f * p.b_frame_pitch;
    long long acc[4][4] = {};                                                   // [channel][|d|, d^2, max, changed]
    for (int i = first + (int)threadIdx.x; i < last; i += kThreads) {
        const int y = i / p.W, x = i - y * p.W;
        const uint8_t* const pa = fa + y * p.a_row_pitch + (int64_t)x * p.bpp;
        const uint8_t* const pb = fb + y * p.b_row_pitch + (int64_t)x * p.bpp;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c < p.bpp) {
                const int d = abs((int)pa[c] - (int)pb[c]);
                acc[c][0] += d; acc[c][1] += d * d; acc[c][2] = max(acc[c][2], (long long)d); acc[c][3] += d != 0;
            }
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long v = k == 2 ? wave_max(acc[c][k]) : wave_sum(acc[c][k]);
            if (lane == 0) part[wave][c * 4 + k] = v;
        }
    }
    __syncthreads();
    const int slot = threadIdx.x;
    if (slot < 4 * p.bpp) {
        long long v = part[0][slot];
        unsigned long long* const out = p.sums + ((int64_t)f * p.bpp) * 4 + slot;
        if ((slot & 3) == 2) {
#pragma unroll
            for (int w = 1; w < kWaves; ++w) v = max(v, part[w][slot]);
            atomicMax(out, (unsigned long long)v);
        } else {
#pragma unroll
            for (int w = 1; w < kWaves; ++w) v += part[w][slot];
            atomicAdd(out, (unsigned long long)v);
        }
    }
}

__global__ void __launch_bounds__(kThreads) ssim_kernel(const PairArgs p)
{
    __shared__ uint8_t ta[kInH][kInW * 4], tb[kInH][kInW * 4];                  // 2 x 4368 bytes
    __shared__ RowSums hb;
    __shared__ long long part[kWaves];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & (kWave - 1);
    const int f = blockIdx.x / (unsigned)p.per_frame;
    const int tile = blockIdx.x - f * p.per_frame;
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const int oh = p.H - kHalo, ow = p.W - kHalo;
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    const int tw = min(kTileW, ow - x0), th = min(kTileH, oh - y0);             // 1 .. 32, 1 .. 16
    const int ih = th + kHalo, row_bytes = (tw + kHalo) * p.bpp;                // <= 26, <= 168
    const uint8_t* const fa = p.a + f * p.a_frame_pitch + y0 * p.a_row_pitch + (int64_t)x0 * p.bpp;
    const uint8_t* const fb = p.b + f * p.b_frame_pitch + y0 * p.b_row_pitch + (int64_t)x0 * p.bpp;
    for (int i = tid; i < ih * row_bytes; i += kThreads) {
        const int r = i / row_bytes, c = i - r * row_bytes;
        ta[r][c] = fa[r * p.a_row_pitch + c];
        tb[r][c] = fb[r * p.b_row_pitch + c];
    }
    __syncthreads();
    for (int c = 0; c < p.bpp; ++c) {
        for (int i = tid; i < ih * kTileW; i += kThreads) {                     // the horizontal pass
            const int r = i >> 5, x = i & (kTileW - 1);
            if (x < tw) {
                int s[5] = {};
#pragma unroll
                for (int k = 0; k < kTaps; ++k) row_tap(s, ta[r][(x + k) * p.bpp + c], tb[r][(x + k) * p.bpp + c], k);
                put_row_sums(hb, r, x, s);
            }
        }
        __syncthreads();
        long long mine = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {                                           // the vertical pass: window (x, y) of the tile
            const int o = tid + j * kThreads, y = o >> 5, x = o & (kTileW - 1);
            if (y < th && x < tw) {
                Moments m{0, 0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < kTaps; ++k) column_tap(m, hb, y, x, k);
                const double q = window_values<false>(m);
                mine += contribution(q);
                if (p.map) p.map[(((int64_t)f * oh + y0 + y) * ow + x0 + x) * p.bpp + c] = (float)q;
            }
        }
        mine = wave_sum(mine);
        if (lane == 0) part[wave] = mine;
        __syncthreads();                                                        // (also: every read of hb came before the next channel's writes)
        if (tid == 0) {
            long long total = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) total += part[w];
            unsigned long long* const out = p.sums + ((int64_t)f * p.bpp + c) * 2;
            atomicAdd(out, (unsigned long long)total);
            atomicAdd(out + 1, (unsigned long long)(tw * th));
        }
        __syncthreads();                                                        // part is free again
    }
}

} // namespace

extern "C" int p3d_video_error_sums(const uint8_t* a, int64_t a_frame_pitch, int64_t a_row_pitch, const uint8_t* b, int64_t b_frame_pitch,
                                    int64_t b_row_pitch, int32_t n_frames, int32_t h, int32_t w, int32_t bpp, int64_t* sums, p3d_stream_t stream)
{
    using namespace p3d;
    int64_t pixels = 0;
    const int rc = check_pair("video_error_sums", a, a_frame_pitch, a_row_pitch, b, b_frame_pitch, b_row_pitch, n_frames, h, w, bpp, sums, &pixels);
    if (rc != P3D_OK || pixels == 0) return rc;
    PairArgs p{a, a_frame_pitch, a_row_pitch, b, b_frame_pitch, b_row_pitch, h, w, bpp, 0, 0, (unsigned long long*)sums, nullptr};
    p.per_frame = ceil_div((int64_t)h * w, kErrPixels);
    const int64_t groups = (int64_t)n_frames * p.per_frame;                    // < 2^31, as the pixels are
    hipLaunchKernelGGL(error_sums_kernel, dim3((unsigned)groups), dim3(kThreads), 0, (hipStream_t)stream, p);
    count_launch(FAM_AUX);
    return check_launch("video_error_sums");
}

extern "C" int p3d_video_ssim(const uint8_t* a, int64_t a_frame_pitch, int64_t a_row_pitch, const uint8_t* b, int64_t b_frame_pitch, int64_t b_row_pitch,
                              int32_t n_frames, int32_t h, int32_t w, int32_t bpp, int64_t* sums, float* map, p3d_stream_t stream)
{
    using namespace p3d;
    int64_t pixels = 0;
    const int rc = check_pair("video_ssim", a, a_frame_pitch, a_row_pitch, b, b_frame_pitch, b_row_pitch, n_frames, h, w, bpp, sums, &pixels);
    if (rc != P3D_OK || pixels == 0 || h < kTaps || w < kTaps) return rc;
    P3D_REQUIRE(((uintptr_t)map & 3u) == 0, "video_ssim: map must be 4-byte aligned");
    PairArgs p{a, a_frame_pitch, a_row_pitch, b, b_frame_pitch, b_row_pitch, h, w, bpp, 0, 0, (unsigned long long*)sums, map};
    p.tiles_x = ceil_div(w - kHalo, kTileW);
    p.per_frame = p.tiles_x * ceil_div(h - kHalo, kTileH);
    const int64_t groups = (int64_t)n_frames * p.per_frame;
    hipLaunchKernelGGL(ssim_kernel, dim3((unsigned)groups), dim3(kThreads), 0, (hipStream_t)stream, p);
    count_launch(FAM_AUX);
    return check_launch("video_ssim");
}
