// Reading lossless frames back: RFC 1951 inflate and the inverse of the PNG row filters (p3d_video.h, "the way back from a lossless file";
// pix2pix3d_amd/video/png_read.py).
//
// p3d_video_png_inflate   a lane owns one PART — a run of whole deflate blocks that begins on a byte — and inflates it into its own range of the output:
//                         Huffman decoding is a chain of data-dependent shifts and a match reads what the part has just written, so the parallel unit is
//                         the part.  The routine is png_inflate.h, the text a host program runs under the sanitizers.  A part's decode state — the code
//                         lengths, and per code the number of codes of every length and the symbols in code order — is 528 16-bit words.  It sits in
//                         LDS, word i of lane l at [i * 32 + l]: lanes that walk their tables in step read neighbouring words.  32 lanes a work-group
//                         are 33 792 bytes, so four work-groups share a CU's 160 KB; 64 lanes would need more than the 64 KB a work-group may have.
//                         The output is zeroed by one asynchronous fill before the launch.
// p3d_video_png_unfilter  a skewed wavefront.  A work-group of one wave owns a frame and walks it in bands of 64 rows; lane r owns row r of the band and
//                         runs one pixel behind lane r - 1, so that at step t it reconstructs pixel t - r: the byte above (b) is what the lane above
//                         finished one step ago — one cross-lane move of the 8-byte pixel register —, the byte above-left (c) is the b of the step
//                         before, the byte to the left (a) the lane's own last pixel.  A band costs w + 63 steps whatever types its rows chose; Sub and
//                         Up would run faster alone, but one schedule serves every mix of types and keeps the dependences of Average and Paeth in
//                         registers.  The row above a band's first is read back from the output after a fence.  The next step's residuals are loaded
//                         before the current pixel is reconstructed, so the loads stay off the chain.
#include "../p3d_common.h"
#include "p3d_video.h"
#include "png_inflate.h"

namespace {

using namespace p3d;

static_assert(png::kBlockType == P3D_VIDEO_PNG_STATUS_BLOCK_TYPE && png::kStored == P3D_VIDEO_PNG_STATUS_STORED &&
              png::kCodeLengths == P3D_VIDEO_PNG_STATUS_CODE_LENGTHS && png::kNoCode == P3D_VIDEO_PNG_STATUS_NO_CODE &&
              png::kDistance == P3D_VIDEO_PNG_STATUS_DISTANCE && png::kOverflow == P3D_VIDEO_PNG_STATUS_OVERFLOW &&
              png::kExhausted == P3D_VIDEO_PNG_STATUS_EXHAUSTED && png::kLeftover == P3D_VIDEO_PNG_STATUS_LEFTOVER &&
              png::kBoundary == P3D_VIDEO_PNG_STATUS_BOUNDARY && png::kShort == P3D_VIDEO_PNG_STATUS_SHORT && png::kFilter == P3D_VIDEO_PNG_STATUS_FILTER &&
              png::kAdler == P3D_VIDEO_PNG_STATUS_ADLER, "png_inflate.h and p3d_video.h agree");
constexpr int kLanes = P3D_VIDEO_PNG_INFLATE_LANES;
static_assert(kLanes * png::kStateHalves * 2 <= 65536, "a work-group's decode state fits its LDS");

struct InflateArgs {
    const uint8_t* data; int64_t data_bytes;
    const int64_t* parts; int n_parts;
    uint8_t* out; int64_t out_bytes;
    int32_t* status;
};

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ void __launch_bounds__(kLanes) png_inflate_kernel(const InflateArgs a)
{
    __shared__ uint16_t state[png::kStateHalves * kLanes];
    const int lane = threadIdx.x;
    const int64_t part = (int64_t)blockIdx.x * kLanes + lane;
    if (part >= a.n_parts) return;                                             // (no barrier below)
    const int64_t* const p = a.parts + 5 * part;
    const int64_t in_begin = clamp64(p[0], 0, a.data_bytes), in_end = clamp64(p[1], in_begin, a.data_bytes);
    const int64_t out_begin = clamp64(p[2], 0, a.out_bytes), out_end = clamp64(p[3], out_begin, a.out_bytes);
    const png::State s = {state + lane, kLanes};
    a.status[part] = png::inflate_part(a.data, in_begin, in_end, a.out, out_begin, out_end, p[4] != 0, s);
}

struct UnfilterArgs {
    const uint8_t* filtered;
    int H, W, bpp;
    uint8_t* frames; int64_t frame_pitch, row_pitch;
    int32_t* status;
};

__device__ __forceinline__ uint64_t load_pixel(const uint8_t* p, int bpp)
{
    uint64_t v = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < bpp) v |= (uint64_t)p[j] << (8 * j);
    return v;
}

__global__ void __launch_bounds__(kWave) png_unfilter_kernel(const UnfilterArgs a)
{
    const int lane = threadIdx.x;
    const int64_t f = blockIdx.x;
    const int64_t R = 1 + (int64_t)a.W * a.bpp;
    const uint8_t* const in = a.filtered + f * a.H * R;
    uint8_t* const out = a.frames + f * a.frame_pitch;
    int bad = 0;
    for (int y0 = 0; y0 < a.H; y0 += kWave) {
        const int y = y0 + lane;
        const bool has_row = y < a.H;
        const uint8_t* const row = in + (int64_t)(has_row ? y : 0) * R;
        uint8_t* const dst = out + (int64_t)(has_row ? y : 0) * a.row_pitch;
        int type = has_row ? row[0] : 0;
        if (type > 4) { bad = 1; type = 0; }
        if (y0) { __threadfence(); __syncthreads(); }                          // the band above is written: its last row is this band's row above
        const uint8_t* const above = out + (int64_t)(y0 - 1) * a.row_pitch;     // read by lane 0 only, and only where y0 > 0
        uint64_t left = 0, up_left = 0, mine = 0;                              // pixels: byte j of the pixel at bits 8 j
        uint64_t next = has_row && lane == 0 && a.W > 0 ? load_pixel(row + 1, a.bpp) : 0;
        const int steps = a.W + kWave - 1;
        for (int t = 0; t < steps; ++t) {
            const int x = t - lane;
            const bool on = has_row && x >= 0 && x < a.W;
            const uint64_t residual = next;
            const int xn = x + 1;                                             // the next step's residuals, before this step's arithmetic
            next = has_row && xn >= 0 && xn < a.W ? load_pixel(row + 1 + (int64_t)xn * a.bpp, a.bpp) : 0;
            uint64_t up = __shfl_up(mine, 1);                                  // the lane above finished pixel x one step ago
            if (lane == 0) up = y0 && on ? load_pixel(above + (int64_t)x * a.bpp, a.bpp) : 0;
            if (on) {
                uint64_t v = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (j < a.bpp) {
                        const int r = png::unfilter_byte(type, (int)(residual >> (8 * j)) & 255, (int)(left >> (8 * j)) & 255, (int)(up >> (8 * j)) & 255,
                                                         (int)(up_left >> (8 * j)) & 255);
                        v |= (uint64_t)r << (8 * j);
                        dst[(int64_t)x * a.bpp + j] = (uint8_t)r;
                    }
                left = v; mine = v; up_left = up;
            }
        }
    }
    const unsigned long long any = __ballot(bad);
    if (lane == 0) a.status[f] = any ? P3D_VIDEO_PNG_STATUS_FILTER : 0;
}

} // namespace

extern "C" int p3d_video_png_inflate(const uint8_t* data, int64_t data_bytes, const int64_t* parts, int32_t n_parts, uint8_t* out, int64_t out_bytes,
                                     int32_t* status, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(data_bytes >= 0 && out_bytes >= 0 && n_parts >= 0, "video_png_inflate: data_bytes, out_bytes and n_parts must be >= 0 (got %lld, %lld, %d)",
                (long long)data_bytes, (long long)out_bytes, n_parts);
    P3D_REQUIRE((data || data_bytes == 0) && (out || out_bytes == 0), "video_png_inflate: data and out must be non-null where they have bytes");
    if (n_parts == 0) return P3D_OK;
    P3D_REQUIRE(parts && status && ((uintptr_t)parts & 7u) == 0 && ((uintptr_t)status & 3u) == 0,
                "video_png_inflate: parts and status must be non-null, parts 8-byte aligned and status 4-byte");
    InflateArgs a;
    a.data = data; a.data_bytes = data_bytes; a.parts = parts; a.n_parts = n_parts; a.out = out; a.out_bytes = out_bytes; a.status = status;
    const hipStream_t s = (hipStream_t)stream;
    if (out_bytes && hipMemsetAsync(out, 0, (size_t)out_bytes, s) != hipSuccess) return fail(P3D_ERR_LAUNCH, "video_png_inflate: memset failed");
    count_launch(FAM_AUX);
    hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)((n_parts + kLanes - 1) / kLanes)), dim3(kLanes), 0, s, a);
    count_launch(FAM_AUX);
    return check_launch("video_png_inflate");
}

extern "C" int p3d_video_png_unfilter(const uint8_t* filtered, int32_t n_frames, int32_t h, int32_t w, int32_t bpp, uint8_t* frames, int64_t frame_pitch,
                                      int64_t row_pitch, int32_t* status, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(n_frames >= 0 && h >= 0 && w >= 0, "video_png_unfilter: n_frames, h and w must be >= 0 (got %d, %d, %d)", n_frames, h, w);
    P3D_REQUIRE(bpp >= 1 && bpp <= 8, "video_png_unfilter: bpp must be 1 .. 8 (got %d)", bpp);
    const int64_t n = (int64_t)w * bpp, frame = (int64_t)h * (n + 1);
    P3D_REQUIRE(n < (1ll << 31) && frame < (1ll << 31) && frame * n_frames < (1ll << 31), "video_png_unfilter: %d x %d x %d pixels of %d bytes reach 2^31",
                n_frames, h, w, bpp);
    if ((int64_t)n_frames * h * w == 0) return P3D_OK;
    P3D_REQUIRE(filtered && frames && status && ((uintptr_t)status & 3u) == 0,
                "video_png_unfilter: filtered, frames and status must be non-null, status 4-byte aligned");
    P3D_REQUIRE(row_pitch >= n && frame_pitch >= 0, "video_png_unfilter: the row pitch is shorter than the row, or the frame pitch negative");
    UnfilterArgs a;
    a.filtered = filtered; a.H = h; a.W = w; a.bpp = bpp; a.frames = frames; a.frame_pitch = frame_pitch; a.row_pitch = row_pitch; a.status = status;
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)n_frames), dim3(kWave), 0, (hipStream_t)stream, a);
    count_launch(FAM_AUX);
    return check_launch("video_png_unfilter");
}
