// The edge-map canvas of a sketch session (p3d_sketch.h; pix2pix3d_amd/sketch.py).  Integer rules throughout: every result
// byte (and, for the conditioning image, every float: a table entry) is defined by the header, and the torch formulations of sketch.py produce the same.
//
// p3d_sketch_condition     one thread per output pixel, 64 consecutive pixels of a row per wave: nine clamped-index byte loads around the sampled
//                          source pixel (the blur is never evaluated where the nearest resize does not look), one table read, one float store.
// p3d_sketch_edge_classes  one launch.  A work-group owns a 64 x 16 tile and builds four images of it in LDS, each from the one before:
//                          grey (72 x 24, halo 4: the only global reads), the horizontal [1 4 6 4 1] sums (68 x 24), the smoothed tile (68 x 20,
//                          halo 2), the Sobel pair (66 x 18, halo 1, zero outside the image).  Every LDS image is indexed by ABSOLUTE pixel
//                          position minus the image's origin and a tap reflects its absolute index before it subtracts the origin: the
//                          reflected pixel of a tile at the border lies inside the same tile's halo.  Positions outside the image hold
//                          values nothing reads.  The suppression then reads its neighbours' magnitudes from LDS: no second pass over global memory.
// p3d_sketch_link          memset of the flags, then mark and select, one thread per pixel each.
// p3d_sketch_thin_step     one thread per pixel: eight clamped-index loads, predicates for "inside", one bit of the step's 256-bit table.
#include "../p3d_common.h"
#include "p3d_sketch.h"
#include "thin_table.h"

namespace {

using namespace p3d;

constexpr int kRowsPerBlock = 4;                    // 256 threads = 4 waves = 4 rows of 64 pixels

__device__ __forceinline__ int reflect(int i, int n)
{
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return min(max(i, 0), n - 1);
}

// ---- condition -------------------------------------------------------------------------------------------------------------------
struct CondArgs { const uint8_t* ink; int64_t pitch; const float* table; float* out; int64_t out_pitch; int H, W, R, blur; };

__global__ void __launch_bounds__(256) condition_kernel(const CondArgs a)
{
    const int x = blockIdx.x * kWave + (threadIdx.x & (kWave - 1)), y = blockIdx.y * kRowsPerBlock + threadIdx.x / kWave;
    if (x >= a.R || y >= a.R) return;
    const int sy = min(y * a.H / a.R, a.H - 1), sx = min(x * a.W / a.R, a.W - 1);      // y * H < 2^24
    int m;
    if (a.blur) {
        int sum = 4;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const uint8_t* row = a.ink + (int64_t)reflect(sy + dy, a.H) * a.pitch;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) sum += row[reflect(sx + dx, a.W)];
        }
        m = sum / 9;
    } else {
        m = a.ink[(int64_t)sy * a.pitch + sx];
    }
    a.out[(int64_t)y * a.out_pitch + x] = a.table[m];
}

// ---- edge classes ------------------------------------------------------------------------------------------------------------------
constexpr int kTW = P3D_SKETCH_TILE_W, kTH = P3D_SKETCH_TILE_H;
constexpr int kGW = kTW + 8, kGH = kTH + 8;         // grey: halo 4
constexpr int kSW = kTW + 4, kSH = kTH + 4;         // smoothed: halo 2
constexpr int kMW = kTW + 2, kMH = kTH + 2;         // gradients: halo 1

struct EdgeArgs { const uint8_t* image; int64_t pitch; uint8_t* classes; int64_t classes_pitch; int H, W, low, high; };

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

template <int CH, bool SMOOTH>
__global__ void __launch_bounds__(256) edge_classes_kernel(const EdgeArgs a)
{
    __shared__ uint8_t grey[kGH * kGW];             // pixel (x0 - 4 + i, y0 - 4 + j) at [j][i]
    __shared__ uint16_t hsum[kGH * kSW];            // rows of grey, columns of smooth: <= 16 * 255
    __shared__ uint8_t smooth[kSH * kSW];           // pixel (x0 - 2 + i, y0 - 2 + j)
    __shared__ short gxs[kMH * kMW], gys[kMH * kMW];      // pixel (x0 - 1 + i, y0 - 1 + j); |g| <= 1020

    const int tid = threadIdx.x, x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;

    for (int e = tid; e < kGH * kGW; e += 256) {
        const int j = e / kGW, i = e - j * kGW;
        const int y = clampi(y0 - 4 + j, a.H - 1), x = clampi(x0 - 4 + i, a.W - 1);    // outside the image: a pixel nothing reads
        const uint8_t* p = a.image + (int64_t)y * a.pitch + (int64_t)x * CH;
        grey[e] = CH == 3 ? (uint8_t)((77 * p[0] + 150 * p[1] + 29 * p[2] + 128) >> 8) : p[0];
    }
    __syncthreads();

    if (SMOOTH) {
        for (int e = tid; e < kGH * kSW; e += 256) {
            const int j = e / kSW, i = e - j * kSW;
            const int x = clampi(x0 - 2 + i, a.W - 1);
            const uint8_t* row = grey + j * kGW;
            const int t0 = row[clampi(reflect(x - 2, a.W) - (x0 - 4), kGW - 1)], t1 = row[clampi(reflect(x - 1, a.W) - (x0 - 4), kGW - 1)];
            const int t2 = row[clampi(x - (x0 - 4), kGW - 1)];
            const int t3 = row[clampi(reflect(x + 1, a.W) - (x0 - 4), kGW - 1)], t4 = row[clampi(reflect(x + 2, a.W) - (x0 - 4), kGW - 1)];
            hsum[e] = (uint16_t)(t0 + 4 * t1 + 6 * t2 + 4 * t3 + t4);
        }
        __syncthreads();
        for (int e = tid; e < kSH * kSW; e += 256) {
            const int j = e / kSW, i = e - j * kSW;
            const int y = clampi(y0 - 2 + j, a.H - 1);
            const int t0 = hsum[clampi(reflect(y - 2, a.H) - (y0 - 4), kGH - 1) * kSW + i], t1 = hsum[clampi(reflect(y - 1, a.H) - (y0 - 4), kGH - 1) * kSW + i];
            const int t2 = hsum[clampi(y - (y0 - 4), kGH - 1) * kSW + i];
            const int t3 = hsum[clampi(reflect(y + 1, a.H) - (y0 - 4), kGH - 1) * kSW + i], t4 = hsum[clampi(reflect(y + 2, a.H) - (y0 - 4), kGH - 1) * kSW + i];
            smooth[e] = (uint8_t)((t0 + 4 * t1 + 6 * t2 + 4 * t3 + t4 + 128) >> 8);
        }
    } else {
        for (int e = tid; e < kSH * kSW; e += 256) {
            const int j = e / kSW, i = e - j * kSW;
            smooth[e] = grey[(j + 2) * kGW + i + 2];
        }
    }
    __syncthreads();

    for (int e = tid; e < kMH * kMW; e += 256) {
        const int j = e / kMW, i = e - j * kMW;
        const int y = y0 - 1 + j, x = x0 - 1 + i;
        const bool inside = x >= 0 && x < a.W && y >= 0 && y < a.H;
        const int yc = clampi(y, a.H - 1), xc = clampi(x, a.W - 1);
        const int ju = clampi(reflect(yc - 1, a.H) - (y0 - 2), kSH - 1) * kSW, jc = clampi(yc - (y0 - 2), kSH - 1) * kSW;
        const int jd = clampi(reflect(yc + 1, a.H) - (y0 - 2), kSH - 1) * kSW;
        const int il = clampi(reflect(xc - 1, a.W) - (x0 - 2), kSW - 1), ic = clampi(xc - (x0 - 2), kSW - 1);
        const int ir = clampi(reflect(xc + 1, a.W) - (x0 - 2), kSW - 1);
        const int ul = smooth[ju + il], uc = smooth[ju + ic], ur = smooth[ju + ir];
        const int cl = smooth[jc + il], cr = smooth[jc + ir];
        const int dl = smooth[jd + il], dc = smooth[jd + ic], dr = smooth[jd + ir];
        const int gx = (ur + 2 * cr + dr) - (ul + 2 * cl + dl), gy = (dl + 2 * dc + dr) - (ul + 2 * uc + ur);
        gxs[e] = (short)(inside ? gx : 0);                                      // a magnitude outside the image counts as 0
        gys[e] = (short)(inside ? gy : 0);
    }
    __syncthreads();

    for (int e = tid; e < kTH * kTW; e += 256) {
        const int j = e / kTW, i = e - j * kTW;
        const int y = y0 + j, x = x0 + i;
        if (x >= a.W || y >= a.H) continue;
        const int c = (j + 1) * kMW + i + 1;
        const int gx = gxs[c], gy = gys[c];
        const int ax = abs(gx), mag = ax + abs(gy);
        const int ay = abs(gy) << 15, t22 = ax * 13573, t67 = t22 + (ax << 16);
        int before, after;                                                      // offsets of the two neighbours across the edge
        bool tie_after;                                                         // mag >= the second neighbour (the axis cases) or mag > it
        if (ay < t22)      { before = -1; after = 1; tie_after = true; }
        else if (ay > t67) { before = -kMW; after = kMW; tie_after = true; }
        else { const int s = ((gx ^ gy) < 0) ? -1 : 1; before = -kMW - s; after = kMW + s; tie_after = false; }
        const int mb = abs((int)gxs[c + before]) + abs((int)gys[c + before]), ma = abs((int)gxs[c + after]) + abs((int)gys[c + after]);
        const bool kept = mag > mb && (tie_after ? mag >= ma : mag > ma);
        a.classes[(int64_t)y * a.classes_pitch + x] = (uint8_t)(kept && mag > a.high ? 2 : (kept && mag > a.low ? 1 : 0));
    }
}

// ---- link ------------------------------------------------------------------------------------------------------------------------
struct LinkArgs { const uint8_t* classes; int64_t pitch; const int32_t* ids; int32_t* flag; uint8_t* ink; int64_t ink_pitch; int H, W; };

__global__ void __launch_bounds__(256) link_mark_kernel(const LinkArgs a)
{
    const int x = blockIdx.x * kWave + (threadIdx.x & (kWave - 1)), y = blockIdx.y * kRowsPerBlock + threadIdx.x / kWave;
    if (x >= a.W || y >= a.H) return;
    const int id = a.ids[(int64_t)y * a.W + x];
    if (a.classes[(int64_t)y * a.pitch + x] == 2 && (unsigned)id < (unsigned)(a.H * a.W)) a.flag[id] = 1;
}

__global__ void __launch_bounds__(256) link_select_kernel(const LinkArgs a)
{
    const int x = blockIdx.x * kWave + (threadIdx.x & (kWave - 1)), y = blockIdx.y * kRowsPerBlock + threadIdx.x / kWave;
    if (x >= a.W || y >= a.H) return;
    const int id = a.ids[(int64_t)y * a.W + x];
    const bool known = (unsigned)id < (unsigned)(a.H * a.W);
    const bool on = a.classes[(int64_t)y * a.pitch + x] != 0 && known && a.flag[known ? id : 0] != 0;
    a.ink[(int64_t)y * a.ink_pitch + x] = on ? 255 : 0;
}

// ---- thinning ----------------------------------------------------------------------------------------------------------------------
struct ThinArgs { const uint8_t* src; int64_t pitch; uint8_t* dst; int64_t dst_pitch; unsigned deletable[8]; int H, W, threshold; };

__global__ void __launch_bounds__(256) thin_step_kernel(const ThinArgs a)
{
    const int x = blockIdx.x * kWave + (threadIdx.x & (kWave - 1)), y = blockIdx.y * kRowsPerBlock + threadIdx.x / kWave;
    if (x >= a.W || y >= a.H) return;
    const int xl = max(x - 1, 0), xr = min(x + 1, a.W - 1);
    const uint8_t* row = a.src + (int64_t)y * a.pitch;
    const uint8_t* up = a.src + (int64_t)max(y - 1, 0) * a.pitch;
    const uint8_t* down = a.src + (int64_t)min(y + 1, a.H - 1) * a.pitch;
    const bool top = y > 0, bottom = y < a.H - 1, left = x > 0, right = x < a.W - 1;
    const int t = a.threshold;
    unsigned code = 0;                                                          // N, NE, E, SE, S, SW, W, NW
    code |= (top && up[x] >= t) ? 1u : 0u;
    code |= (top && right && up[xr] >= t) ? 2u : 0u;
    code |= (right && row[xr] >= t) ? 4u : 0u;
    code |= (bottom && right && down[xr] >= t) ? 8u : 0u;
    code |= (bottom && down[x] >= t) ? 16u : 0u;
    code |= (bottom && left && down[xl] >= t) ? 32u : 0u;
    code |= (left && row[xl] >= t) ? 64u : 0u;
    code |= (top && left && up[xl] >= t) ? 128u : 0u;
    const bool set = row[x] >= t, gone = (a.deletable[code >> 5] >> (code & 31)) & 1u;
    a.dst[(int64_t)y * a.dst_pitch + x] = (set && !gone) ? 255 : 0;
}

bool size_ok(int32_t h, int32_t w) { return h >= 1 && w >= 1 && h <= P3D_PAINT_MAX_SIZE && w <= P3D_PAINT_MAX_SIZE; }
dim3 pixel_grid(int32_t h, int32_t w) { return dim3((unsigned)ceil_div(w, kWave), (unsigned)ceil_div(h, kRowsPerBlock)); }

} // namespace

extern "C" int p3d_sketch_condition(const uint8_t* ink, int64_t ink_row_pitch, int32_t h, int32_t w, int32_t blur, const float* table, float* out,
                                    int64_t out_row_pitch, int32_t resolution, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(ink && table && out, "sketch_condition: ink, table and out must be non-null");
    P3D_REQUIRE(size_ok(h, w), "sketch_condition: the canvas is 1 .. %d pixels a side (got %d x %d)", P3D_PAINT_MAX_SIZE, h, w);
    P3D_REQUIRE(resolution >= 1 && resolution <= P3D_PAINT_MAX_SIZE, "sketch_condition: the resolution is 1 .. %d (got %d)", P3D_PAINT_MAX_SIZE, resolution);
    P3D_REQUIRE(ink_row_pitch >= w && out_row_pitch >= resolution, "sketch_condition: a row pitch is shorter than the row");
    P3D_REQUIRE((((uintptr_t)table | (uintptr_t)out) & 3u) == 0, "sketch_condition: table and out must be 4-byte aligned");
    CondArgs a;
    a.ink = ink; a.pitch = ink_row_pitch; a.table = table; a.out = out; a.out_pitch = out_row_pitch; a.H = h; a.W = w; a.R = resolution; a.blur = blur != 0;
    hipLaunchKernelGGL(condition_kernel, pixel_grid(resolution, resolution), dim3(256), 0, (hipStream_t)stream, a);
    count_launch(FAM_AUX);
    return check_launch("sketch_condition");
}

extern "C" int p3d_sketch_edge_classes(const uint8_t* image, int64_t image_row_pitch, int32_t channels, uint8_t* classes, int64_t classes_row_pitch,
                                       int32_t h, int32_t w, int32_t low, int32_t high, int32_t smooth, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(image && classes, "sketch_edge_classes: image and classes must be non-null");
    P3D_REQUIRE(size_ok(h, w), "sketch_edge_classes: the image is 1 .. %d pixels a side (got %d x %d)", P3D_PAINT_MAX_SIZE, h, w);
    P3D_REQUIRE(channels == 1 || channels == 3, "sketch_edge_classes: channels is 1 (grey) or 3 (RGB) (got %d)", channels);
    P3D_REQUIRE(image_row_pitch >= (int64_t)channels * w && classes_row_pitch >= w, "sketch_edge_classes: a row pitch is shorter than the row");
    P3D_REQUIRE(0 <= low && low <= high && high <= P3D_SKETCH_MAX_MAGNITUDE, "sketch_edge_classes: 0 <= low <= high <= %d is needed (got %d, %d)",
                P3D_SKETCH_MAX_MAGNITUDE, low, high);
    P3D_REQUIRE((const uint8_t*)classes != image, "sketch_edge_classes: the classes are written out of place");
    EdgeArgs a;
    a.image = image; a.pitch = image_row_pitch; a.classes = classes; a.classes_pitch = classes_row_pitch; a.H = h; a.W = w; a.low = low; a.high = high;
    const dim3 grid((unsigned)ceil_div(w, kTW), (unsigned)ceil_div(h, kTH));
    const hipStream_t s = (hipStream_t)stream;
    if (channels == 3) {
        if (smooth) hipLaunchKernelGGL((edge_classes_kernel<3, true>), grid, dim3(256), 0, s, a);
        else        hipLaunchKernelGGL((edge_classes_kernel<3, false>), grid, dim3(256), 0, s, a);
    } else {
        if (smooth) hipLaunchKernelGGL((edge_classes_kernel<1, true>), grid, dim3(256), 0, s, a);
        else        hipLaunchKernelGGL((edge_classes_kernel<1, false>), grid, dim3(256), 0, s, a);
    }
    count_launch(FAM_AUX);
    return check_launch("sketch_edge_classes");
}

extern "C" int p3d_sketch_link(const uint8_t* classes, int64_t classes_row_pitch, const int32_t* ids, int32_t* flag, uint8_t* ink, int64_t ink_row_pitch,
                               int32_t h, int32_t w, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(classes && ids && flag && ink, "sketch_link: classes, ids, flag and ink must be non-null");
    P3D_REQUIRE(size_ok(h, w), "sketch_link: the image is 1 .. %d pixels a side (got %d x %d)", P3D_PAINT_MAX_SIZE, h, w);
    P3D_REQUIRE(classes_row_pitch >= w && ink_row_pitch >= w, "sketch_link: a row pitch is shorter than the row");
    P3D_REQUIRE((((uintptr_t)ids | (uintptr_t)flag) & 3u) == 0, "sketch_link: ids and flag must be 4-byte aligned");
    P3D_REQUIRE((const void*)ids != (const void*)flag && (const uint8_t*)ink != classes, "sketch_link: the workspace must not be ids, nor the ink the classes");
    LinkArgs a;
    a.classes = classes; a.pitch = classes_row_pitch; a.ids = ids; a.flag = flag; a.ink = ink; a.ink_pitch = ink_row_pitch; a.H = h; a.W = w;
    const hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(flag, 0, sizeof(int32_t) * (size_t)h * w, s) != hipSuccess) return fail(P3D_ERR_LAUNCH, "sketch_link: memset failed");
    hipLaunchKernelGGL(link_mark_kernel, pixel_grid(h, w), dim3(256), 0, s, a);
    count_launch(FAM_AUX);
    hipLaunchKernelGGL(link_select_kernel, pixel_grid(h, w), dim3(256), 0, s, a);
    count_launch(FAM_AUX);
    return check_launch("sketch_link");
}

extern "C" int p3d_sketch_thin_step(const uint8_t* src, int64_t src_row_pitch, uint8_t* dst, int64_t dst_row_pitch, int32_t h, int32_t w, int32_t threshold,
                                    int32_t step, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(src && dst, "sketch_thin_step: src and dst must be non-null");
    P3D_REQUIRE(size_ok(h, w), "sketch_thin_step: the image is 1 .. %d pixels a side (got %d x %d)", P3D_PAINT_MAX_SIZE, h, w);
    P3D_REQUIRE(src_row_pitch >= w && dst_row_pitch >= w, "sketch_thin_step: a row pitch is shorter than the row");
    P3D_REQUIRE(threshold >= 1 && threshold <= 255, "sketch_thin_step: the threshold is 1 .. 255 (got %d)", threshold);
    P3D_REQUIRE(step == 0 || step == 1, "sketch_thin_step: step is 0 or 1 (got %d)", step);
    P3D_REQUIRE((const uint8_t*)dst != src, "sketch_thin_step: the image is written out of place");
    ThinArgs a;
    a.src = src; a.pitch = src_row_pitch; a.dst = dst; a.dst_pitch = dst_row_pitch; a.H = h; a.W = w; a.threshold = threshold;
    for (int k = 0; k < 8; ++k) a.deletable[k] = kThinDeletable[step][k];
    hipLaunchKernelGGL(thin_step_kernel, pixel_grid(h, w), dim3(256), 0, (hipStream_t)stream, a);
    count_launch(FAM_AUX);
    return check_launch("sketch_thin_step");
}
