// The SSIM window on the device: what ssim_kernel of video_quality.hip and msssim_level_kernel of frame_multiscale.hip both run, in the integers
// p3d_video.h states.  Device code only, no entry point.  A work-group of kThreads lanes owns up to kTileW x kTileH windows of one frame; the kernels stage
// the kInW x kInH samples under them in LDS each in its own way (bytes in one, shifted dwords in the other) and then, per channel:
//
//     row_tap           the horizontal pass, a tap at a time: the five int32 row sums A, B, Pxx, Pyy, Pxy of one (input row, window column), which
//                       put_row_sums stores to hb — a barrier follows, the caller's;
//     column_tap        the vertical pass of one window, a tap at a time: a lane reads down its own column of hb (consecutive lanes, consecutive words:
//                       no bank conflict);
//     window_values     the header's four int64 factors and q = (n1 n2) / (d1 d2) in fp64, and with CS the second value cs = n2 / d2 — a template
//                       parameter, so that a kernel that does not ask for cs holds no division for it;
//     contribution      llrint(value 2^32), what a window adds to a sum;
//     wave_sum          the reduction the contributions meet in.
//
// The two loops over the taps are the kernels': `#pragma unroll for (int k = 0; k < kTaps; ++k)`.  Unrolled in the kernel a pass stays a chain of
// multiply-adds with one operand live at a time.  Unrolled inside a helper it does not: the helper is optimised before it is inlined, the compiler pairs
// the taps of equal weight first, and the kernels measured 2 % slower with the horizontal pass so and needed twice the VGPRs with the vertical one so.
//
// fp rules: contraction is off where a value is made, the four conversions round to nearest even and every operator rounds once.
#ifndef P3D_SSIM_WINDOW_H
#define P3D_SSIM_WINDOW_H
#include "../p3d_common.h"
#include "p3d_video.h"

namespace p3d {
namespace ssim {

constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr int kTaps = P3D_VIDEO_SSIM_TAPS, kHalo = kTaps - 1;
constexpr int kTileW = P3D_VIDEO_SSIM_TILE_W, kTileH = P3D_VIDEO_SSIM_TILE_H;   // windows of a work-group
constexpr int kInW = kTileW + kHalo, kInH = kTileH + kHalo;                     // the samples under them: 42 x 26
constexpr long long kC1 = P3D_VIDEO_SSIM_C1, kC2 = P3D_VIDEO_SSIM_C2;
static_assert(kTileW * kTileH == 2 * kThreads && kTileW == 32, "two windows a lane, a row of windows half a wave");
static_assert(P3D_VIDEO_SSIM_SHIFT == 32, "a window contributes llrint(value 2^32)");

using RowSums = int[5][kInH][kTileW];                                           // 16640 bytes of LDS: A, B, Pxx, Pyy, Pxy of (input row, window column)

struct Moments {
    int A, B;                                                                   // < 2^28
    long long Pxx, Pyy, Pxy;                                                    // < 2^36
};

__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d);
    return v;                                                                   // lane 0 holds the sum
}

// Tap k = 0 .. kTaps - 1 of the horizontal pass into zeroed sums: xa and xb are the channel's samples of the two clips k pixels right of the window's first.
__device__ __forceinline__ void row_tap(int (&s)[5], int xa, int xb, int k)     // every sum <= 1024 x 255^2 < 2^26
{
    constexpr int g[kTaps] = {P3D_VIDEO_SSIM_WINDOW};
    s[0] += g[k] * xa; s[1] += g[k] * xb;
    s[2] += g[k] * xa * xa; s[3] += g[k] * xb * xb; s[4] += g[k] * xa * xb;
}

__device__ __forceinline__ void put_row_sums(RowSums& hb, int r, int x, const int (&s)[5])
{
#pragma unroll
    for (int m = 0; m < 5; ++m) hb[m][r][x] = s[m];
}

// Tap k = 0 .. kTaps - 1 of the vertical pass of the window (x, y) of the tile, into zeroed moments.
__device__ __forceinline__ void column_tap(Moments& m, const RowSums& hb, int y, int x, int k)
{
    constexpr int g[kTaps] = {P3D_VIDEO_SSIM_WINDOW};
    m.A += g[k] * hb[0][y + k][x]; m.B += g[k] * hb[1][y + k][x];
    m.Pxx += (long long)g[k] * hb[2][y + k][x]; m.Pyy += (long long)g[k] * hb[3][y + k][x]; m.Pxy += (long long)g[k] * hb[4][y + k][x];
}

// One window's value q from its five moments and, with CS, the second value into *cs.
template <bool CS>
__device__ __forceinline__ double window_values(const Moments& m, double* cs = nullptr)
{
#pragma clang fp contract(off)
    const long long A = m.A, B = m.B;
    const long long ab = A * B, aa_bb = A * A + B * B;
    const long long n1 = 2 * ab + kC1, n2 = 2 * ((m.Pxy << 20) - ab) + kC2;
    const long long d1 = aa_bb + kC1, d2 = ((m.Pxx + m.Pyy) << 20) - aa_bb + kC2;
    const double fn2 = (double)n2, fd2 = (double)d2;
    const double num = (double)n1 * fn2;
    const double den = (double)d1 * fd2;
    if (CS) *cs = fn2 / fd2;
    return num / den;
}

__device__ __forceinline__ long long contribution(double value)
{
    return llrint(value * 4294967296.0);
}

} // namespace ssim
} // namespace p3d
#endif
