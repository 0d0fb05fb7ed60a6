// Frame resampling for gfx950: the two passes of Pillow's Image.resize on 8-bit clips and the nearest gather (p3d_video.h, "frame resampling";
// pix2pix3d_amd/resample.py).  The rules are the header's; the torch formulation of resample.py produces the same bytes.
//
// All three kernels are 256 threads a work-group — 64 lanes along a row by 4 waves, a wave taking every fourth row of the tile's
// P3D_RESAMPLE_TILE_H — with the frames on grid.z (strided when there are more than 65535).  Every offset is 64-bit.  Whatever a table holds is
// clamped into the axis before it is used (axis_bounds, the nearest indices), so no load leaves a source row; every store is guarded by the
// output's own sizes.
//
// p3d_frame_resample_rows      a lane owns one output pixel (all its bytes) of four rows.  The tile's 64 (xmin, count) pairs and 64 weight rows go to
//                              LDS once a work-group; per frame the source span [lo, hi) of the tile's 16 rows is staged in LDS — dwords where
//                              the global address allows, the LDS copy keeping the address's low two bits so that an aligned dword stays
//                              aligned — and every tap is an LDS byte read.  The weight of a tap is read once for the lane's four rows.  A span
//                              or a tap list too long for LDS is read from global memory directly (the same loop on other pointers).
// p3d_frame_resample_columns   a lane owns four consecutive bytes of a row, a wave one output row at a time: bounds and weights are scalar loads
//                              and the source rows are read as coalesced dwords (256 bytes a wave); bytes where a row's address or tail
//                              does not allow a dword.  No LDS: the rows neighbouring outputs share are re-read from L2.
// p3d_frame_resample_nearest   a lane owns one output pixel of four rows; both index tables are read per lane / per wave.
#include "../p3d_common.h"
#include "p3d_video.h"

namespace {

using namespace p3d;

constexpr int kBlock = 256;
constexpr int kTileW = P3D_RESAMPLE_TILE_W, kTileH = P3D_RESAMPLE_TILE_H;
constexpr int kWaves = kBlock / 64, kRowsPerWave = kTileH / kWaves;
constexpr int kLdsTaps = P3D_RESAMPLE_LDS_TAPS, kLdsRowBytes = P3D_RESAMPLE_LDS_ROW_BYTES;
constexpr int kWeightStride = kLdsTaps + 1;                    // dwords: an odd stride spreads the 64 weight rows over the banks
constexpr int kRowStride = kLdsRowBytes / 4 + 1;               // dwords: the span plus the up to 3 bytes that keep the address's alignment
constexpr int kHalf = 1 << 21, kShift = 22;
constexpr int kMaxGridZ = 65535;
static_assert(kTileW == 64 && kTileH % kWaves == 0 && kLdsRowBytes % 4 == 0, "a wave spans the tile's width");

struct Clip { const uint8_t* src; int64_t sfp, srp; uint8_t* dst; int64_t dfp, drp; int frames, h, w; };

// (xmin, count) of output `o`, clamped into an axis of n entries and a table of ksize taps.
__device__ __forceinline__ void axis_bounds(const int32_t* __restrict__ bounds, int o, int n, int ksize, int& first, int& count)
{
    int a = bounds[2 * (int64_t)o], c = bounds[2 * (int64_t)o + 1];
    a = a < 0 ? 0 : (a > n ? n : a);
    const int room = n - a < ksize ? n - a : ksize;
    first = a;
    count = c < 0 ? 0 : (c > room ? room : c);
}

__device__ __forceinline__ uint8_t clip8(int acc)
{
    const int v = acc >> kShift;                               // arithmetic on int32
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// The sums of one output pixel of a lane's rows: the weight of a tap is read once for all of them.
template <int BPP>
__device__ __forceinline__ void tap_sums(const int32_t* __restrict__ taps, int count, const uint8_t* const (&row)[kRowsPerWave],
                                         int (&acc)[kRowsPerWave][BPP])
{
    for (int j = 0; j < kRowsPerWave; ++j)
        for (int c = 0; c < BPP; ++c) acc[j][c] = kHalf;
    for (int i = 0; i < count; ++i) {
        const int k = taps[i];
#pragma unroll
        for (int j = 0; j < kRowsPerWave; ++j)
#pragma unroll
            for (int c = 0; c < BPP; ++c) acc[j][c] += k * (int)row[j][i * BPP + c];
    }
}

// ---- the horizontal pass ------------------------------------------------------------------------------------------------------------------
template <int BPP>
__global__ void __launch_bounds__(kBlock) resample_rows_kernel(Clip g, int ow, const int32_t* __restrict__ bounds, const int32_t* __restrict__ weights,
                                                               int ksize)
{
    __shared__ int32_t s_first[kTileW], s_count[kTileW];
    __shared__ int32_t s_span[2];
    __shared__ int32_t s_weights[kTileW * kWeightStride];
    __shared__ uint32_t s_rows[kTileH * kRowStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const int xx = x0 + lane;
    const int columns = ow - x0 < kTileW ? ow - x0 : kTileW;   // >= 1
    if (wave == 0) {
        int first = 0, count = 0;
        if (lane < columns) axis_bounds(bounds, xx, g.w, ksize, first, count);
        s_first[lane] = first;
        s_count[lane] = count;
        int lo = count > 0 ? first : g.w, hi = count > 0 ? first + count : 0;
        for (int m = 32; m > 0; m >>= 1) {
            const int lo2 = __shfl_xor(lo, m), hi2 = __shfl_xor(hi, m);
            lo = lo2 < lo ? lo2 : lo;
            hi = hi2 > hi ? hi2 : hi;
        }
        if (lane == 0) { s_span[0] = hi > lo ? lo : 0; s_span[1] = hi > lo ? hi : 0; }
    }
    __syncthreads();
    const int lo = s_span[0], hi = s_span[1];
    const int span_bytes = (hi - lo) * BPP;                    // <= w * 4
    const bool staged = ksize <= kLdsTaps && span_bytes <= kLdsRowBytes;      // the same for the whole work-group
    if (staged)
        for (int idx = threadIdx.x; idx < columns * ksize; idx += kBlock)      // the tile's weight rows are one contiguous run
            s_weights[(idx / ksize) * kWeightStride + idx % ksize] = weights[(int64_t)x0 * ksize + idx];
    const int first = s_first[lane], count = lane < columns ? s_count[lane] : 0;

    for (int f = blockIdx.z; f < g.frames; f += gridDim.z) {
        const uint8_t* frame = g.src + (int64_t)f * g.sfp;
        if (staged) {
            __syncthreads();                                   // the previous frame's taps are read; the weights are written
            for (int j = 0; j < kRowsPerWave; ++j) {
                const int r = wave + j * kWaves, y = y0 + r;
                if (y >= g.h) break;
                const uint8_t* a = frame + (int64_t)y * g.srp + (int64_t)lo * BPP;
                const int shift = (int)((uintptr_t)a & 3u);
                for (int d = lane; d * 4 < shift + span_bytes; d += 64) {
                    const int b0 = d * 4 - shift;              // the span's byte that is byte 0 of this dword
                    uint32_t v = 0;
                    if (b0 >= 0 && b0 + 4 <= span_bytes) {
                        v = *reinterpret_cast<const uint32_t*>(a + b0);
                    } else {
                        for (int b = 0; b < 4; ++b)
                            if (b0 + b >= 0 && b0 + b < span_bytes) v |= (uint32_t)a[b0 + b] << (8 * b);
                    }
                    s_rows[r * kRowStride + d] = v;
                }
            }
            __syncthreads();
        }
        if (lane >= columns) continue;                         // (no barrier follows inside this iteration)
        int acc[kRowsPerWave][BPP];
        const uint8_t* row[kRowsPerWave];                      // byte 0 of the tap list of this lane's pixel, per row
        if (staged) {
            for (int j = 0; j < kRowsPerWave; ++j) {
                const int r = wave + j * kWaves;
                const int y = y0 + r < g.h ? y0 + r : g.h - 1; // a row past the image was not staged: its sums are never stored
                const int shift = (int)((uintptr_t)(frame + (int64_t)y * g.srp + (int64_t)lo * BPP) & 3u);
                row[j] = reinterpret_cast<const uint8_t*>(s_rows) + (r * kRowStride * 4 + shift + (first - lo) * BPP);
            }
            tap_sums<BPP>(s_weights + lane * kWeightStride, count, row, acc);
        } else {
            for (int j = 0; j < kRowsPerWave; ++j) {
                const int r = wave + j * kWaves;
                const int y = y0 + r < g.h ? y0 + r : g.h - 1; // a row past the image reads the last one and stores nothing
                row[j] = frame + (int64_t)y * g.srp + (int64_t)first * BPP;
            }
            tap_sums<BPP>(weights + (int64_t)xx * ksize, count, row, acc);
        }
        for (int j = 0; j < kRowsPerWave; ++j) {
            const int y = y0 + wave + j * kWaves;
            if (y >= g.h) break;
            uint8_t* out = g.dst + (int64_t)f * g.dfp + (int64_t)y * g.drp + (int64_t)xx * BPP;
            for (int c = 0; c < BPP; ++c) out[c] = clip8(acc[j][c]);
        }
    }
}

// ---- the vertical pass -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) resample_columns_kernel(Clip g, int64_t row_bytes, int oh, const int32_t* __restrict__ bounds,
                                                                  const int32_t* __restrict__ weights, int ksize)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);       // scalar: the row, its bounds and its weights are wave-uniform
    const int64_t j0 = ((int64_t)blockIdx.x * kTileW + lane) * 4;
    if (j0 >= row_bytes) return;
    const int nb = row_bytes - j0 < 4 ? (int)(row_bytes - j0) : 4;
    for (int f = blockIdx.z; f < g.frames; f += gridDim.z) {
        const uint8_t* frame = g.src + (int64_t)f * g.sfp;
        for (int j = 0; j < kRowsPerWave; ++j) {
            const int yy = blockIdx.y * kTileH + wave + j * kWaves;
            if (yy >= oh) break;
            int first, count;
            axis_bounds(bounds, yy, g.h, ksize, first, count);
            const int32_t* taps = weights + (int64_t)yy * ksize;
            int acc[4] = {kHalf, kHalf, kHalf, kHalf};
            for (int i = 0; i < count; ++i) {
                const int k = taps[i];
                const uint8_t* srow = frame + (int64_t)(first + i) * g.srp;
                uint32_t v = 0;
                if (nb == 4 && ((uintptr_t)srow & 3u) == 0) {
                    v = *reinterpret_cast<const uint32_t*>(srow + j0);
                } else {
                    for (int b = 0; b < nb; ++b) v |= (uint32_t)srow[j0 + b] << (8 * b);
                }
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[b] += k * (int)((v >> (8 * b)) & 0xffu);
            }
            uint8_t* drow = g.dst + (int64_t)f * g.dfp + (int64_t)yy * g.drp;
            if (nb == 4 && ((uintptr_t)drow & 3u) == 0) {
                *reinterpret_cast<uint32_t*>(drow + j0) = (uint32_t)clip8(acc[0]) | ((uint32_t)clip8(acc[1]) << 8) | ((uint32_t)clip8(acc[2]) << 16) |
                                                          ((uint32_t)clip8(acc[3]) << 24);
            } else {
                for (int b = 0; b < nb; ++b) drow[j0 + b] = clip8(acc[b]);
            }
        }
    }
}

// ---- the gather ----------------------------------------------------------------------------------------------------------------------
template <int BPP>
__global__ void __launch_bounds__(kBlock) resample_nearest_kernel(Clip g, int oh, int ow, const int32_t* __restrict__ x_index,
                                                                  const int32_t* __restrict__ y_index)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int xx = blockIdx.x * kTileW + lane;
    if (xx >= ow) return;
    int sx = x_index[xx];
    sx = sx < 0 ? 0 : (sx > g.w - 1 ? g.w - 1 : sx);
    for (int f = blockIdx.z; f < g.frames; f += gridDim.z)
        for (int j = 0; j < kRowsPerWave; ++j) {
            const int yy = blockIdx.y * kTileH + wave + j * kWaves;
            if (yy >= oh) break;
            int sy = y_index[yy];
            sy = sy < 0 ? 0 : (sy > g.h - 1 ? g.h - 1 : sy);
            const uint8_t* in = g.src + (int64_t)f * g.sfp + (int64_t)sy * g.srp + (int64_t)sx * BPP;
            uint8_t* out = g.dst + (int64_t)f * g.dfp + (int64_t)yy * g.drp + (int64_t)xx * BPP;
            for (int c = 0; c < BPP; ++c) out[c] = in[c];
        }
}

bool size_ok(int32_t n) { return n >= 1 && n <= P3D_RESAMPLE_MAX_SIZE; }

// The shared argument checks: source [frames][h][w][bpp], destination [frames][oh][ow][bpp].  0: fine.
int check_clips(const char* who, const uint8_t* src, int64_t sfp, int64_t srp, int32_t frames, int32_t h, int32_t w, int32_t bpp, const uint8_t* dst,
                int64_t dfp, int64_t drp, int32_t oh, int32_t ow)
{
    P3D_REQUIRE(frames >= 0, "%s: frames must not be negative (got %d)", who, frames);
    P3D_REQUIRE(bpp >= 1 && bpp <= 4, "%s: bpp is 1 .. 4 (got %d)", who, bpp);
    P3D_REQUIRE(size_ok(h) && size_ok(w) && size_ok(oh) && size_ok(ow), "%s: every size is 1 .. %d (got %d x %d -> %d x %d)", who, P3D_RESAMPLE_MAX_SIZE,
                w, h, ow, oh);
    if (frames == 0) return P3D_OK;
    P3D_REQUIRE(src && dst, "%s: a clip pointer is null", who);
    const int64_t src_row = (int64_t)w * bpp, dst_row = (int64_t)ow * bpp;
    P3D_REQUIRE(srp >= src_row && drp >= dst_row, "%s: a row pitch is below its row (%lld < %lld or %lld < %lld)", who, (long long)srp, (long long)src_row,
                (long long)drp, (long long)dst_row);
    const int64_t src_frame = (int64_t)(h - 1) * srp + src_row, dst_frame = (int64_t)(oh - 1) * drp + dst_row;
    P3D_REQUIRE(sfp >= 0 && (frames == 1 || dfp >= dst_frame), "%s: the source's frame pitch must not be negative and the destination's frames must not overlap",
                who);
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)((int64_t)(frames - 1) * sfp + src_frame);
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)((int64_t)(frames - 1) * (frames == 1 ? 0 : dfp) + dst_frame);
    P3D_REQUIRE(d1 <= s0 || s1 <= d0, "%s writes out of place: the destination's bytes meet the source's", who);
    return P3D_OK;
}

dim3 tiles(int64_t across, int32_t rows, int32_t frames)
{
    return dim3((unsigned)((across + kTileW - 1) / kTileW), (unsigned)((rows + kTileH - 1) / kTileH), (unsigned)(frames < kMaxGridZ ? frames : kMaxGridZ));
}

} // namespace

extern "C" int p3d_frame_resample_rows(const uint8_t* src, int64_t src_frame_pitch, int64_t src_row_pitch, int32_t frames, int32_t h, int32_t w, int32_t bpp,
                                       uint8_t* dst, int64_t dst_frame_pitch, int64_t dst_row_pitch, int32_t ow, const int32_t* bounds,
                                       const int32_t* weights, int32_t ksize, p3d_stream_t stream)
{
    using namespace p3d;
    if (int code = check_clips("frame_resample_rows", src, src_frame_pitch, src_row_pitch, frames, h, w, bpp, dst, dst_frame_pitch, dst_row_pitch, h, ow))
        return code;
    P3D_REQUIRE(ksize >= 1, "frame_resample_rows: ksize must be at least 1 (got %d)", ksize);
    if (frames == 0) return P3D_OK;
    P3D_REQUIRE(bounds && weights, "frame_resample_rows: a table pointer is null");
    const Clip g{src, src_frame_pitch, src_row_pitch, dst, dst_frame_pitch, dst_row_pitch, frames, h, w};
    const dim3 grid = tiles(ow, h, frames);
    switch (bpp) {
    case 1: hipLaunchKernelGGL(resample_rows_kernel<1>, grid, dim3(kBlock), 0, (hipStream_t)stream, g, ow, bounds, weights, ksize); break;
    case 2: hipLaunchKernelGGL(resample_rows_kernel<2>, grid, dim3(kBlock), 0, (hipStream_t)stream, g, ow, bounds, weights, ksize); break;
    case 3: hipLaunchKernelGGL(resample_rows_kernel<3>, grid, dim3(kBlock), 0, (hipStream_t)stream, g, ow, bounds, weights, ksize); break;
    default: hipLaunchKernelGGL(resample_rows_kernel<4>, grid, dim3(kBlock), 0, (hipStream_t)stream, g, ow, bounds, weights, ksize); break;
    }
    count_launch(FAM_AUX);
    return check_launch("frame_resample_rows");
}

extern "C" int p3d_frame_resample_columns(const uint8_t* src, int64_t src_frame_pitch, int64_t src_row_pitch, int32_t frames, int32_t h, int32_t w,
                                          int32_t bpp, uint8_t* dst, int64_t dst_frame_pitch, int64_t dst_row_pitch, int32_t oh, const int32_t* bounds,
                                          const int32_t* weights, int32_t ksize, p3d_stream_t stream)
{
    using namespace p3d;
    if (int code = check_clips("frame_resample_columns", src, src_frame_pitch, src_row_pitch, frames, h, w, bpp, dst, dst_frame_pitch, dst_row_pitch, oh, w))
        return code;
    P3D_REQUIRE(ksize >= 1, "frame_resample_columns: ksize must be at least 1 (got %d)", ksize);
    if (frames == 0) return P3D_OK;
    P3D_REQUIRE(bounds && weights, "frame_resample_columns: a table pointer is null");
    const Clip g{src, src_frame_pitch, src_row_pitch, dst, dst_frame_pitch, dst_row_pitch, frames, h, w};
    const int64_t row_bytes = (int64_t)w * bpp;
    hipLaunchKernelGGL(resample_columns_kernel, tiles((row_bytes + 3) / 4, oh, frames), dim3(kBlock), 0, (hipStream_t)stream, g, row_bytes, oh, bounds,
                       weights, ksize);
    count_launch(FAM_AUX);
    return check_launch("frame_resample_columns");
}

extern "C" int p3d_frame_resample_nearest(const uint8_t* src, int64_t src_frame_pitch, int64_t src_row_pitch, int32_t frames, int32_t h, int32_t w,
                                          int32_t bpp, uint8_t* dst, int64_t dst_frame_pitch, int64_t dst_row_pitch, int32_t oh, int32_t ow,
                                          const int32_t* x_index, const int32_t* y_index, p3d_stream_t stream)
{
    using namespace p3d;
    if (int code = check_clips("frame_resample_nearest", src, src_frame_pitch, src_row_pitch, frames, h, w, bpp, dst, dst_frame_pitch, dst_row_pitch, oh, ow))
        return code;
    if (frames == 0) return P3D_OK;
    P3D_REQUIRE(x_index && y_index, "frame_resample_nearest: an index table pointer is null");
    const Clip g{src, src_frame_pitch, src_row_pitch, dst, dst_frame_pitch, dst_row_pitch, frames, h, w};
    const dim3 grid = tiles(ow, oh, frames);
    switch (bpp) {
    case 1: hipLaunchKernelGGL(resample_nearest_kernel<1>, grid, dim3(kBlock), 0, (hipStream_t)stream, g, oh, ow, x_index, y_index); break;
    case 2: hipLaunchKernelGGL(resample_nearest_kernel<2>, grid, dim3(kBlock), 0, (hipStream_t)stream, g, oh, ow, x_index, y_index); break;
    case 3: hipLaunchKernelGGL(resample_nearest_kernel<3>, grid, dim3(kBlock), 0, (hipStream_t)stream, g, oh, ow, x_index, y_index); break;
    default: hipLaunchKernelGGL(resample_nearest_kernel<4>, grid, dim3(kBlock), 0, (hipStream_t)stream, g, oh, ow, x_index, y_index); break;
    }
    count_launch(FAM_AUX);
    return check_launch("frame_resample_nearest");
}
