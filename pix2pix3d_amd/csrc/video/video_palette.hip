// Palette, dither and index frames for the GIF writer (p3d_video.h; pix2pix3d_amd/video/gif.py).  Integer rules throughout:
// every result is defined by the header, and the torch formulations of video/gif.py produce the same bytes.
//
// p3d_video_histogram    a work-group of 1024 threads owns a share of one frame's pixels and the whole 32768-bin histogram in LDS (128 KB: one
//                        work-group per CU).  A wave takes 64 consecutive pixels; lanes whose bin equals their left neighbour's form a run, and
//                        only the first lane of a run adds the run's length (one ballot), so a smooth frame costs a few LDS adds per wave and a
//                        flat one a single add.  The non-zero bins are then added to the group's counts with global integer atomics.  Integer
//                        adds commute: any order gives the same counts.
// p3d_video_box_sums     the same shares; the group's 32 KB bin -> box lookup and 256 x 4 uint32 accumulators sit in LDS (a share is at most
//                        2^20 pixels, so a sum stays below 2^28).  A wave whose 64 pixels fall into ONE box reduces them across the lanes and adds
//                        once; any other wave adds per lane.  One flush of int64 atomics per work-group.
// p3d_video_quantize     a thread owns four consecutive pixels of a row.  The palette sits in LDS as {-512 r, -512 g, -512 b, (r^2+g^2+b^2) << 8 | k}:
//                        key_k = 256 (d_k^2 - |p|^2) + k is three multiply-adds on it, and min over k of key_k orders by (d^2, k) — the nearest row,
//                        the lowest on a tie, with no compare-and-select.  The LDS read is the same address for the whole wave (a broadcast) and
//                        serves the thread's four pixels.
#include "../p3d_common.h"
#include "p3d_video.h"

namespace {

using namespace p3d;

constexpr int kBins = P3D_VIDEO_BINS, kColors = P3D_VIDEO_COLORS;
constexpr int kShareThreads = 1024;                 // histogram and box sums: 16 waves around one LDS table
constexpr int kMinShare = 16384, kMaxShare = 1 << 20;      // pixels of a frame per work-group: enough to pay for the flush; few enough for uint32 sums

struct ClipArgs {
    const uint8_t* frames; int64_t frame_pitch, row_pitch;
    int W, HW;                                      // pixels of a row, of a frame
    int shares, share;                              // work-groups per frame, pixels per work-group (the last one of a frame takes the rest)
    int per_frame;
};

// The pixel `p` of frame `f` (p < HW): its three bytes.
__device__ __forceinline__ void load_pixel(const ClipArgs& a, int f, unsigned p, unsigned& r, unsigned& g, unsigned& b)
{
    const unsigned y = p / (unsigned)a.W, x = p - y * (unsigned)a.W;
    const uint8_t* const px = a.frames + (int64_t)f * a.frame_pitch + (int64_t)y * a.row_pitch + 3 * (int64_t)x;
    r = px[0]; g = px[1]; b = px[2];
}

__global__ void __launch_bounds__(256) zero_kernel(int32_t* dst, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = 0;
}

__global__ void __launch_bounds__(kShareThreads) histogram_kernel(const ClipArgs a, int32_t* __restrict__ counts)
{
    __shared__ int bins[kBins];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    for (int i = tid; i < kBins; i += kShareThreads) bins[i] = 0;
    __syncthreads();
    const int f = blockIdx.x / a.shares, c = blockIdx.x - f * a.shares;
    const unsigned begin = (unsigned)c * (unsigned)a.share, end = min(begin + (unsigned)a.share, (unsigned)a.HW);
    for (unsigned base = begin; base < end; base += kShareThreads) {
        const unsigned p = base + tid;
        const bool valid = p < end;
        unsigned r, g, b;
        load_pixel(a, f, min(p, end - 1), r, g, b);                       // lanes past the share re-read its last pixel and add nothing
        const int bin = valid ? (int)(((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3)) : -1;
        const int left = __shfl_up(bin, 1);
        const bool start = lane == 0 || bin != left;
        const unsigned long long later = (__ballot(start) >> lane) >> 1;    // run starts after this lane
        const int length = later ? __ffsll(later) : kWave - lane;
        if (start && valid) atomicAdd(&bins[bin], length);
    }
    __syncthreads();
    int32_t* const dst = counts + (a.per_frame ? (int64_t)f * kBins : 0);
    for (int i = tid; i < kBins; i += kShareThreads) {
        const int v = bins[i];
        if (v) atomicAdd(dst + i, v);
    }
}

__global__ void __launch_bounds__(kShareThreads) box_sums_kernel(const ClipArgs a, const uint8_t* __restrict__ box_of_bin, int64_t* __restrict__ sums)
{
    __shared__ unsigned lookup[kBins / 4];
    __shared__ unsigned acc[kColors * 4];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int f = blockIdx.x / a.shares, c = blockIdx.x - f * a.shares;
    const int64_t group = a.per_frame ? f : 0;
    const unsigned* const src = (const unsigned*)(box_of_bin + group * kBins);
    for (int i = tid; i < kBins / 4; i += kShareThreads) lookup[i] = src[i];
    acc[tid] = 0;                                                             // kColors * 4 == kShareThreads
    __syncthreads();
    const uint8_t* const box_of = (const uint8_t*)lookup;
    const unsigned begin = (unsigned)c * (unsigned)a.share, end = min(begin + (unsigned)a.share, (unsigned)a.HW);
    for (unsigned base = begin; base < end; base += kShareThreads) {
        const unsigned p = base + tid;
        const bool valid = p < end;
        unsigned r, g, b;
        load_pixel(a, f, min(p, end - 1), r, g, b);                       // lanes past the share re-read its last pixel: its box, and zeros to add
        const int box = box_of[((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3)];
        unsigned n = valid ? 1u : 0u;
        r = valid ? r : 0u; g = valid ? g : 0u; b = valid ? b : 0u;
        const int first = __builtin_amdgcn_readfirstlane(box);
        if (__ballot(box != first) == 0ull) {                              // one box for the whole wave: reduce across the lanes, add once
#pragma unroll
            for (int m = kWave / 2; m >= 1; m >>= 1) {
                r += __shfl_xor(r, m); g += __shfl_xor(g, m); b += __shfl_xor(b, m); n += __shfl_xor(n, m);
            }
            if (lane == 0 && n) {
                atomicAdd(&acc[first * 4 + 0], r); atomicAdd(&acc[first * 4 + 1], g); atomicAdd(&acc[first * 4 + 2], b); atomicAdd(&acc[first * 4 + 3], n);
            }
        } else if (valid) {
            atomicAdd(&acc[box * 4 + 0], r); atomicAdd(&acc[box * 4 + 1], g); atomicAdd(&acc[box * 4 + 2], b); atomicAdd(&acc[box * 4 + 3], 1u);
        }
    }
    __syncthreads();
    const unsigned v = acc[tid];
    if (v) atomicAdd((unsigned long long*)(sums + group * (kColors * 4) + tid), (unsigned long long)v);
}

struct QuantArgs {
    ClipArgs clip;
    const uint8_t* palette; const int32_t* n_colors;
    uint8_t* out; int64_t out_frame_pitch, out_row_pitch;
    int quads_per_row, quads, blocks_per_frame, amplitude;
};

__global__ void __launch_bounds__(256) quantize_kernel(const QuantArgs a)
{
    __shared__ int4 rows[kColors];
    __shared__ int offsets[64];
    const int tid = threadIdx.x;
    const int f = blockIdx.x / a.blocks_per_frame, c = blockIdx.x - f * a.blocks_per_frame;
    const int64_t group = a.clip.per_frame ? f : 0;
    const int n = min(max(a.n_colors[group], 1), kColors);
    {
        const uint8_t* const row = a.palette + (group * kColors + tid) * 3;
        const int r = row[0], g = row[1], b = row[2];
        rows[tid] = tid < n ? make_int4(-512 * r, -512 * g, -512 * b, ((r * r + g * g + b * b) << 8) | tid) : make_int4(0, 0, 0, 0x7fffffff);
    }
    if (tid < 64) {
        const int x = tid & 7, y = tid >> 3;
        const int q0 = 2 * ((x ^ y) & 1) + (y & 1), q1 = 2 * (((x ^ y) >> 1) & 1) + ((y >> 1) & 1), q2 = 2 * (((x ^ y) >> 2) & 1) + ((y >> 2) & 1);
        offsets[tid] = ((2 * (16 * q0 + 4 * q1 + q2) - 63) * a.amplitude) >> 7;
    }
    __syncthreads();

    const int q = c * 256 + tid;
    const bool valid = q < a.quads;
    const int qc = min(q, a.quads - 1);                                       // threads past the frame re-read its last quad and store nothing
    const int y = qc / a.quads_per_row, x0 = 4 * (qc - y * a.quads_per_row);
    const uint8_t* const src = a.clip.frames + (int64_t)f * a.clip.frame_pitch + (int64_t)y * a.clip.row_pitch;
    int pr[4], pg[4], pb[4], best[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint8_t* const px = src + 3 * (int64_t)min(x0 + i, a.clip.W - 1);
        const int off = offsets[(y & 7) * 8 + ((x0 + i) & 7)];
        pr[i] = min(max((int)px[0] + off, 0), 255);
        pg[i] = min(max((int)px[1] + off, 0), 255);
        pb[i] = min(max((int)px[2] + off, 0), 255);
        best[i] = 0x7fffffff;
    }
    const int n4 = (n + 3) & ~3;                                              // rows n .. n4 - 1 hold the largest key: they never win
    for (int k = 0; k < n4; k += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int4 row = rows[k + j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                best[i] = min(best[i], row.w + __mul24(pr[i], row.x) + __mul24(pg[i], row.y) + __mul24(pb[i], row.z));
        }
    }
    uint8_t* const dst = a.out + (int64_t)f * a.out_frame_pitch + (int64_t)y * a.out_row_pitch + x0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (valid && x0 + i < a.clip.W) dst[i] = (uint8_t)(best[i] & 255);
}

// The checks every entry point shares, and the split of the clip into work-groups.  `pixels` = n_frames * h * w.
int clip_args(const char* what, const uint8_t* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n_frames, int32_t h, int32_t w,
              int32_t per_frame, ClipArgs* a, int64_t* pixels)
{
    P3D_REQUIRE(n_frames >= 0 && h >= 0 && w >= 0, "%s: n_frames, h and w must be >= 0 (got %d, %d, %d)", what, n_frames, h, w);
    P3D_REQUIRE(per_frame == 0 || per_frame == 1, "%s: per_frame is 0 or 1 (got %d)", what, per_frame);
    const int64_t hw = (int64_t)h * w;
    P3D_REQUIRE(hw < (1ll << 31) && hw * n_frames < (1ll << 31), "%s: %d x %d x %d pixels reach 2^31", what, n_frames, h, w);
    *pixels = hw * n_frames;
    if (*pixels == 0) return P3D_OK;
    P3D_REQUIRE(frames, "%s: frames must be non-null", what);
    P3D_REQUIRE(row_pitch >= 3 * (int64_t)w && frame_pitch >= 0, "%s: the row pitch is shorter than the row, or the frame pitch negative", what);
    a->frames = frames; a->frame_pitch = frame_pitch; a->row_pitch = row_pitch; a->W = w; a->HW = (int)hw; a->per_frame = per_frame;
    const int64_t wanted = (hw + kMinShare - 1) / kMinShare, room = 1024 / n_frames > 1 ? 1024 / n_frames : 1, needed = (hw + kMaxShare - 1) / kMaxShare;
    const int64_t shares = wanted < room ? wanted : (room > needed ? room : needed);
    a->share = (int)((hw + shares - 1) / shares);
    a->shares = (int)((hw + a->share - 1) / a->share);                        // no share is empty
    return P3D_OK;
}

void zero(int32_t* dst, int64_t n, hipStream_t s)
{
    if (n == 0) return;
    hipLaunchKernelGGL(zero_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, dst, n);
    count_launch(FAM_AUX);
}

} // namespace

extern "C" int p3d_video_histogram(const uint8_t* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n_frames, int32_t h, int32_t w,
                                   int32_t per_frame, int32_t* counts, p3d_stream_t stream)
{
    using namespace p3d;
    ClipArgs a;
    int64_t pixels = 0;
    const int rc = clip_args("video_histogram", frames, frame_pitch, row_pitch, n_frames, h, w, per_frame, &a, &pixels);
    if (rc != P3D_OK) return rc;
    const int64_t groups = per_frame ? n_frames : 1;
    P3D_REQUIRE(groups == 0 || (counts && ((uintptr_t)counts & 3u) == 0), "video_histogram: counts must be non-null and 4-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    zero(counts, groups * kBins, s);
    if (pixels) {
        hipLaunchKernelGGL(histogram_kernel, dim3((unsigned)(n_frames * a.shares)), dim3(kShareThreads), 0, s, a, counts);
        count_launch(FAM_AUX);
    }
    return check_launch("video_histogram");
}

extern "C" int p3d_video_box_sums(const uint8_t* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n_frames, int32_t h, int32_t w,
                                  int32_t per_frame, const uint8_t* box_of_bin, int64_t* sums, p3d_stream_t stream)
{
    using namespace p3d;
    ClipArgs a;
    int64_t pixels = 0;
    const int rc = clip_args("video_box_sums", frames, frame_pitch, row_pitch, n_frames, h, w, per_frame, &a, &pixels);
    if (rc != P3D_OK) return rc;
    const int64_t groups = per_frame ? n_frames : 1;
    P3D_REQUIRE(groups == 0 || (sums && ((uintptr_t)sums & 7u) == 0), "video_box_sums: sums must be non-null and 8-byte aligned");
    P3D_REQUIRE(pixels == 0 || (box_of_bin && ((uintptr_t)box_of_bin & 3u) == 0), "video_box_sums: box_of_bin must be non-null and 4-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    zero((int32_t*)sums, groups * kColors * 4 * 2, s);
    if (pixels) {
        hipLaunchKernelGGL(box_sums_kernel, dim3((unsigned)(n_frames * a.shares)), dim3(kShareThreads), 0, s, a, box_of_bin, sums);
        count_launch(FAM_AUX);
    }
    return check_launch("video_box_sums");
}

extern "C" int p3d_video_quantize(const uint8_t* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n_frames, int32_t h, int32_t w,
                                  int32_t per_frame, const uint8_t* palette, const int32_t* n_colors, int32_t amplitude, uint8_t* indices,
                                  int64_t index_frame_pitch, int64_t index_row_pitch, p3d_stream_t stream)
{
    using namespace p3d;
    QuantArgs a;
    int64_t pixels = 0;
    const int rc = clip_args("video_quantize", frames, frame_pitch, row_pitch, n_frames, h, w, per_frame, &a.clip, &pixels);
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(amplitude >= 0 && amplitude <= P3D_VIDEO_MAX_AMPLITUDE, "video_quantize: amplitude is 0 .. %d (got %d)", P3D_VIDEO_MAX_AMPLITUDE, amplitude);
    if (pixels == 0) return P3D_OK;
    P3D_REQUIRE(palette && n_colors && indices, "video_quantize: palette, n_colors and indices must be non-null");
    P3D_REQUIRE(((uintptr_t)n_colors & 3u) == 0, "video_quantize: n_colors must be 4-byte aligned");
    P3D_REQUIRE(index_row_pitch >= w && (n_frames == 1 || index_frame_pitch >= (int64_t)h * index_row_pitch),
                "video_quantize: the index rows or frames overlap (pitches %lld, %lld for %d x %d)", (long long)index_frame_pitch, (long long)index_row_pitch, h, w);
    a.palette = palette; a.n_colors = n_colors; a.out = indices; a.out_frame_pitch = index_frame_pitch; a.out_row_pitch = index_row_pitch;
    a.quads_per_row = (w + 3) / 4; a.quads = h * a.quads_per_row; a.blocks_per_frame = ceil_div(a.quads, 256); a.amplitude = amplitude;
    hipLaunchKernelGGL(quantize_kernel, dim3((unsigned)(n_frames * a.blocks_per_frame)), dim3(256), 0, (hipStream_t)stream, a);
    count_launch(FAM_AUX);
    return check_launch("video_quantize");
}
