// Cross-view consistency: the forward warp between cameras (p3d_regions.h states the rules; pix2pix3d_amd/reproject.py).
// Every result is a pure function of the inputs: the projection is fp64 with one rounding per operator in a fixed order (no contraction, no
// sqrt, no rint; fp64 division is correctly rounded), the z-test is a 64-bit integer minimum of (zkey, index) keys and the counters are 64-bit
// integer sums, so the torch formulations of reproject.py produce the same bytes.
//
// p3d_view_splat                  one launch.  One thread per source point; the frames are walked by blockIdx.y, so the 25 camera floats are
//                                 uniform over a work-group.  A point's footprint is 1, 9 or 25 target pixels.  Straight to the z-buffer, all of
//                                 them are read first (independent plain loads), and a cell that already shows a key no larger takes no atomic
//                                 (keys only decrease: a stale read costs a redundant atomic, never a wrong byte); the others take ONE no-return
//                                 signed 64-bit global atomic minimum each.  Neighbouring source pixels land on neighbouring target pixels, so a
//                                 wave's atomics are near-contiguous.  Radius 0 does just that.  Radius 1 and 2 were bound by the rate of the
//                                 global atomics at 512 x 512 (nine footprints overlap on a cell), so a work-group takes a 16 x 16 tile of source
//                                 pixels and, where those land within 32 x 32 cells, takes the minimum in LDS first: one global atomic per
//                                 covered cell.  A tile that lands wider goes straight to the z-buffer.
// p3d_view_resolve                one launch.  One thread per target pixel: the key's index gathers the source bytes, the key's depth is
//                                 compared with the depth of the target view's own point.  The five status counts go by ballot into five LDS
//                                 slots (one LDS add per wave and status that occurs), folded once per work-group.
// p3d_view_difference_histogram   one launch; a 256-slot uint32 histogram per work-group in LDS.  Bin 0 — the common one between consistent
//                                 views — is counted by a ballot per channel and added by one lane; the others by LDS atomics.  One fold per
//                                 work-group, non-zero slots only.
#include "../p3d_common.h"
#include "p3d_regions.h"

#pragma clang fp contract(off)

namespace {

using namespace p3d;

constexpr int kCamFloats = 25, kBlock = 256;
constexpr int kGridX = 64, kGridY = 32768;          // resolve and histogram: a work-group walks <= 2 frames and <= 2^18 pixels of each, so its uint32 LDS
                                                    // counters cannot wrap.  Few work-groups on purpose: each folds its counters into the SAME few global words,
                                                    // and those atomics serialise (resolve at [4, 512, 512] with counts: 30 us at 64 a frame, 53 us at 1024)
constexpr int kSplatGridX = 2048;                   // the splat keeps no counters: a point per thread up to 724 x 724 points a frame
constexpr int kSrcTile = 16, kBoxSide = 32;         // radius > 0: kSrcTile^2 = kBlock source pixels a work-group, staged in LDS where they land within kBoxSide^2 cells (8 KB)
constexpr long long kEmpty = P3D_VIEW_EMPTY;
constexpr double kKeyScale = 65536.0, kKeyLimit = 2147483648.0, kGuard = P3D_VIEW_GUARD;

struct Camera { double m[12], k0, k1, k2, k4, k5; };      // the three rows of cam2world (rotation and translation) and the five intrinsics used

__device__ __forceinline__ Camera load_camera(const float* __restrict__ c)
{
    Camera cam;
#pragma unroll
    for (int i = 0; i < 12; ++i) cam.m[i] = (double)c[i];
    cam.k0 = (double)c[16]; cam.k1 = (double)c[17]; cam.k2 = (double)c[18]; cam.k4 = (double)c[20]; cam.k5 = (double)c[21];
    return cam;
}

struct Projected { double sx, sy, zs; bool ok; };         // zs = zc * 65536; ok: finite, in front of the camera and below the key limit

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) <= 3.40282346638528859812e+38f; }

__device__ __forceinline__ Projected project(const Camera& cam, float fx, float fy, float fz, double W, double H)
{
    const double qx = (double)fx - cam.m[3], qy = (double)fy - cam.m[7], qz = (double)fz - cam.m[11];
    double xc = cam.m[0] * qx; xc = xc + cam.m[4] * qy; xc = xc + cam.m[8] * qz;
    double yc = cam.m[1] * qx; yc = yc + cam.m[5] * qy; yc = yc + cam.m[9] * qz;
    double zc = cam.m[2] * qx; zc = zc + cam.m[6] * qy; zc = zc + cam.m[10] * qz;
    double a = cam.k0 * xc; a = a + cam.k1 * yc;
    const double u = a / zc + cam.k2;
    const double v = (cam.k4 * yc) / zc + cam.k5;
    Projected p;
    p.sx = floor(u * W);
    p.sy = floor(v * H);
    p.zs = zc * kKeyScale;
    p.ok = finite32(fx) && finite32(fy) && finite32(fz) && zc > 0.0 && p.zs < kKeyLimit;
    return p;
}

// ---- splat -------------------------------------------------------------------------------------------------------------------------
struct SplatArgs {
    const float* points; int64_t p_frame;
    const uint8_t* valid; int64_t v_row, v_frame;
    const float* cameras;
    long long* zbuf;
    int frames, h, w, H, W;
};

struct Landed { int sx, sy; long long key; bool keep; };      // where a point lands, its key, and whether it is kept (not dropped)

__device__ __forceinline__ Landed land(const SplatArgs& a, const Camera& cam, const float* __restrict__ pts, const uint8_t* __restrict__ valid, int x, int y)
{
    Landed l;
    l.sx = l.sy = 0; l.key = 0; l.keep = false;
    if (valid && valid[(int64_t)y * a.v_row + x] == 0) return l;
    const int i = y * a.w + x;                                                                   // < 2^24
    const Projected p = project(cam, pts[(int64_t)i * 3], pts[(int64_t)i * 3 + 1], pts[(int64_t)i * 3 + 2], (double)a.W, (double)a.H);
    if (!(p.ok && p.sx >= -kGuard && p.sx < (double)a.W + kGuard && p.sy >= -kGuard && p.sy < (double)a.H + kGuard)) return l;
    l.sx = (int)p.sx; l.sy = (int)p.sy;                                                          // -4 .. W + 3: exact
    l.key = (long long)(((unsigned long long)(long long)floor(p.zs) << 32) | (unsigned)i);
    l.keep = true;
    return l;
}

// The footprint of one kept point straight into the frame's z-buffer.  Pass 1: every cell is read (a cell outside the image reads the nearest one
// inside and is not kept): the loads do not depend on each other.  Pass 2: an atomic where the read showed a larger key.
template <int R>
__device__ __forceinline__ void footprint_global(const SplatArgs& a, long long* __restrict__ zb, const Landed& l)
{
    constexpr int D = 2 * R + 1;
    unsigned need = 0u;
#pragma unroll
    for (int dy = 0; dy < D; ++dy)
#pragma unroll
        for (int dx = 0; dx < D; ++dx) {
            const int ty = l.sy - R + dy, tx = l.sx - R + dx;
            const bool inside = (unsigned)ty < (unsigned)a.H && (unsigned)tx < (unsigned)a.W;
            const long long seen = zb[(int64_t)min(max(ty, 0), a.H - 1) * a.W + min(max(tx, 0), a.W - 1)];
            if (inside && seen > l.key) need |= 1u << (dy * D + dx);
        }
#pragma unroll
    for (int dy = 0; dy < D; ++dy)
#pragma unroll
        for (int dx = 0; dx < D; ++dx)
            if ((need >> (dy * D + dx)) & 1u) atomicMin(zb + (int64_t)(l.sy - R + dy) * a.W + (l.sx - R + dx), l.key);      // inside the frame
}

// radius 0: a point per thread, rows of points in order
__global__ void __launch_bounds__(kBlock) view_splat_kernel(const SplatArgs a)
{
    const int64_t frame_cells = (int64_t)a.H * a.W;
    const int n = a.h * a.w;                                                                     // <= 2^24
    for (int f = blockIdx.y; f < a.frames; f += gridDim.y) {
        const Camera cam = load_camera(a.cameras + (int64_t)f * kCamFloats);
        const float* const pts = a.points + (int64_t)f * a.p_frame;
        const uint8_t* const valid = a.valid ? a.valid + (int64_t)f * a.v_frame : nullptr;
        long long* const zb = a.zbuf + (int64_t)f * frame_cells;
        for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
            const int y = i / a.w;
            const Landed l = land(a, cam, pts, valid, i - y * a.w, y);
            if (l.keep) footprint_global<0>(a, zb, l);
        }
    }
}

// radius 1 and 2: a work-group takes a kSrcTile x kSrcTile tile of source pixels.  Their footprints overlap (a cell is covered by up to 9 or 25 of
// them), so where the tile's landing box fits kBoxSide x kBoxSide cells the minimum is first taken in LDS and every covered cell then costs ONE global
// atomic; a tile that lands wider than that (a depth edge, a magnifying warp) goes straight to the z-buffer.  The minimum is the same either way.
template <int R>
__global__ void __launch_bounds__(kBlock) view_splat_tiled_kernel(const SplatArgs a)
{
    constexpr int D = 2 * R + 1;
    __shared__ long long box_cells[kBoxSide * kBoxSide];
    __shared__ int box[4];                                                                       // min sx, min sy, max sx, max sy of the kept points
    const int tid = threadIdx.x;
    const int tiles_x = (a.w + kSrcTile - 1) / kSrcTile, tiles = tiles_x * ((a.h + kSrcTile - 1) / kSrcTile);
    const int64_t frame_cells = (int64_t)a.H * a.W;
    for (int f = blockIdx.y; f < a.frames; f += gridDim.y) {
        const Camera cam = load_camera(a.cameras + (int64_t)f * kCamFloats);
        const float* const pts = a.points + (int64_t)f * a.p_frame;
        const uint8_t* const valid = a.valid ? a.valid + (int64_t)f * a.v_frame : nullptr;
        long long* const zb = a.zbuf + (int64_t)f * frame_cells;
        for (int t = blockIdx.x; t < tiles; t += gridDim.x) {                                    // uniform over the work-group: every lane reaches the barriers
            const int tile_y = t / tiles_x;
            const int x = (t - tile_y * tiles_x) * kSrcTile + (tid % kSrcTile), y = tile_y * kSrcTile + tid / kSrcTile;
            Landed l;
            l.sx = l.sy = 0; l.key = 0; l.keep = false;
            if (x < a.w && y < a.h) l = land(a, cam, pts, valid, x, y);
            if (tid < 4) box[tid] = tid < 2 ? INT_MAX : INT_MIN;
            __syncthreads();
            if (l.keep) {
                atomicMin(box + 0, l.sx); atomicMin(box + 1, l.sy);
                atomicMax(box + 2, l.sx); atomicMax(box + 3, l.sy);
            }
            __syncthreads();
            const bool any = box[0] <= box[2];
            const int x0 = any ? box[0] - R : 0, y0 = any ? box[1] - R : 0;                      // the landing box: ex x ey cells from (x0, y0)
            const int ex = any ? box[2] - box[0] + D : 0, ey = any ? box[3] - box[1] + D : 0;
            if (any && ex <= kBoxSide && ey <= kBoxSide) {
                for (int c = tid; c < ex * ey; c += kBlock) box_cells[c] = kEmpty;
                __syncthreads();
                if (l.keep) {
#pragma unroll
                    for (int dy = 0; dy < D; ++dy)
#pragma unroll
                        for (int dx = 0; dx < D; ++dx)
                            atomicMin(box_cells + (l.sy - R + dy - y0) * ex + (l.sx - R + dx - x0), l.key);      // 0 <= row < ey, 0 <= column < ex
                }
                __syncthreads();
                for (int c = tid; c < ex * ey; c += kBlock) {
                    const long long key = box_cells[c];
                    const int cy = c / ex, gx = x0 + (c - cy * ex), gy = y0 + cy;
                    // (no read first: nearly every covered cell is still empty, and the read would put a second memory latency into the tile's chain)
                    if (key != kEmpty && (unsigned)gx < (unsigned)a.W && (unsigned)gy < (unsigned)a.H) atomicMin(zb + (int64_t)gy * a.W + gx, key);
                }
            } else if (l.keep) {
                footprint_global<R>(a, zb, l);
            }
            __syncthreads();                                                                     // box and box_cells are used again
        }
    }
}

// ---- resolve -----------------------------------------------------------------------------------------------------------------------
struct ResolveArgs {
    const long long* zbuf;
    const uint8_t* src; int64_t s_row, s_frame;
    uint8_t* dst; int64_t d_row, d_frame;
    int32_t* index;
    uint8_t* status;
    const float* target;
    const float* cameras;
    long long tolerance;
    unsigned long long* counts;
    unsigned fill;                                  // the four fill bytes, channel c in bits 8 c ..
    int frames, n, w, C, H, W;
};

__global__ void __launch_bounds__(kBlock) view_resolve_kernel(const ResolveArgs a)
{
    __shared__ unsigned slots[5];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    if (tid < 5) slots[tid] = 0u;
    __syncthreads();
    const int cells = a.H * a.W;                                                                 // <= 2^24
    for (int f = blockIdx.y; f < a.frames; f += gridDim.y) {
        Camera cam;
        if (a.target) cam = load_camera(a.cameras + (int64_t)f * kCamFloats);
        const int64_t frame0 = (int64_t)f * cells;
        const uint8_t* const src = a.src + (int64_t)f * a.s_frame;
        for (int base = blockIdx.x * kBlock; base < cells; base += gridDim.x * kBlock) {         // uniform over the work-group: every lane reaches the ballots
            const int p = base + tid;
            const bool live = p < cells;
            int st = -1;
            if (live) {
                const long long key = a.zbuf[frame0 + p];
                const unsigned i = (unsigned)((unsigned long long)key & 0xffffffffull);
                const long long zk = key >> 32;
                const bool hole = i >= (unsigned)a.n;
                const int ty = p / a.W, tx = p - ty * a.W;
                uint8_t* const d = a.dst + (int64_t)f * a.d_frame + (int64_t)ty * a.d_row + (int64_t)tx * a.C;
                if (hole) {
                    for (int c = 0; c < a.C; ++c) d[c] = (uint8_t)(a.fill >> (8 * c));
                    st = 0;
                } else {
                    const int y = (int)(i / (unsigned)a.w), x = (int)i - y * a.w;
                    const uint8_t* const s = src + (int64_t)y * a.s_row + (int64_t)x * a.C;
                    for (int c = 0; c < a.C; ++c) d[c] = s[c];
                    st = 1;
                    if (a.target) {
                        const float* const t = a.target + (frame0 + p) * 3;
                        const Projected q = project(cam, t[0], t[1], t[2], (double)a.W, (double)a.H);
                        if (!q.ok) {
                            st = 4;
                        } else {
                            const long long zt = (long long)floor(q.zs), diff = zk - zt;
                            st = (diff <= a.tolerance && -diff <= a.tolerance) ? 1 : (zk > zt ? 2 : 3);
                        }
                    }
                }
                if (a.index) a.index[frame0 + p] = hole ? -1 : (int)i;
                a.status[frame0 + p] = (uint8_t)st;
            }
            if (a.counts) {
#pragma unroll
                for (int s = 0; s < 5; ++s) {
                    const unsigned long long votes = __ballot(st == s);
                    if (lane == 0 && votes) atomicAdd(slots + s, (unsigned)__popcll(votes));
                }
            }
        }
    }
    __syncthreads();
    if (a.counts && tid < 5 && slots[tid]) atomicAdd(a.counts + tid, (unsigned long long)slots[tid]);
}

// ---- difference histogram ----------------------------------------------------------------------------------------------------------
struct DiffArgs {
    const uint8_t* a; int64_t a_row, a_frame;
    const uint8_t* b; int64_t b_row, b_frame;
    const uint8_t* where; int64_t w_row, w_frame;
    unsigned long long* hist;
    int frames, C, H, W, match;
};

__global__ void __launch_bounds__(kBlock) view_difference_histogram_kernel(const DiffArgs a)
{
    __shared__ unsigned slots[256];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    slots[tid] = 0u;
    __syncthreads();
    const int cells = a.H * a.W;
    for (int f = blockIdx.y; f < a.frames; f += gridDim.y) {
        const uint8_t* const fa = a.a + (int64_t)f * a.a_frame;
        const uint8_t* const fb = a.b + (int64_t)f * a.b_frame;
        const uint8_t* const fw = a.where ? a.where + (int64_t)f * a.w_frame : nullptr;
        for (int base = blockIdx.x * kBlock; base < cells; base += gridDim.x * kBlock) {         // uniform over the work-group: every lane reaches the ballots
            const int p = base + tid, pc = min(p, cells - 1);
            const int y = pc / a.W, x = pc - y * a.W;
            const bool in = p < cells && (!fw || fw[(int64_t)y * a.w_row + x] == (uint8_t)a.match);
            const uint8_t* const pa = fa + (int64_t)y * a.a_row + (int64_t)x * a.C;
            const uint8_t* const pb = fb + (int64_t)y * a.b_row + (int64_t)x * a.C;
            for (int c = 0; c < a.C; ++c) {                                                      // C is uniform
                const int d = in ? abs((int)pa[c] - (int)pb[c]) : -1;
                const unsigned long long same = __ballot(d == 0);
                if (lane == 0 && same) atomicAdd(slots, (unsigned)__popcll(same));
                if (d > 0) atomicAdd(slots + d, 1u);
            }
        }
    }
    __syncthreads();
    const unsigned v = slots[tid];
    if (v) atomicAdd(a.hist + tid, (unsigned long long)v);
}

bool view_size_ok(int32_t h, int32_t w) { return h >= 1 && w >= 1 && h <= P3D_PAINT_MAX_SIZE && w <= P3D_PAINT_MAX_SIZE; }

bool frames_ok(int32_t frames) { return frames >= 0 && frames <= P3D_LABEL_MAX_FRAMES; }

// rows `row` and frames `frame` bytes apart hold h rows of `bytes` bytes each without overlapping; `broadcast`: a frame pitch of 0 is one frame for all
bool pitches_ok(int64_t row, int64_t frame, int32_t h, int64_t bytes, int32_t frames, bool broadcast)
{
    if (row < bytes) return false;
    if (frame == 0) return broadcast || frames == 1;
    return frames == 1 || frame >= (int64_t)(h - 1) * row + bytes;
}

dim3 view_grid(int64_t cells, int32_t frames, int grid_x)
{
    const int64_t blocks = (cells + kBlock - 1) / kBlock;
    return dim3((unsigned)(blocks < grid_x ? blocks : grid_x), (unsigned)(frames < kGridY ? frames : kGridY));
}

} // namespace

extern "C" int p3d_view_splat(const float* points, int64_t points_frame_pitch, const uint8_t* valid, int64_t valid_row_pitch,
                              int64_t valid_frame_pitch, const float* cameras, int32_t frames, int32_t h, int32_t w, int32_t radius,
                              int64_t* zbuf, int32_t H, int32_t W, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(frames_ok(frames), "view_splat: frames is 0 .. %d (got %d)", P3D_LABEL_MAX_FRAMES, frames);
    P3D_REQUIRE(view_size_ok(h, w) && view_size_ok(H, W), "view_splat: a view is 1 .. %d pixels a side (got %d x %d into %d x %d)",
                P3D_PAINT_MAX_SIZE, h, w, H, W);
    P3D_REQUIRE(radius >= 0 && radius <= P3D_VIEW_MAX_RADIUS, "view_splat: radius is 0, 1 or 2 (got %d)", radius);
    if (frames == 0) return P3D_OK;
    P3D_REQUIRE(points && cameras && zbuf, "view_splat: points, cameras and zbuf must be non-null");
    const int64_t n = (int64_t)h * w;
    P3D_REQUIRE(points_frame_pitch == 0 || points_frame_pitch >= 3 * n, "view_splat: the points' frame pitch is 0 (one source) or >= 3 h w floats");
    P3D_REQUIRE(!valid || pitches_ok(valid_row_pitch, valid_frame_pitch, h, w, frames, true), "view_splat: a pitch of valid is shorter than its row or frame");
    P3D_REQUIRE(((uintptr_t)points & 3u) == 0 && ((uintptr_t)cameras & 3u) == 0 && ((uintptr_t)zbuf & 7u) == 0,
                "view_splat: points and cameras must be 4-byte and zbuf 8-byte aligned");
    SplatArgs a;
    a.points = points; a.p_frame = points_frame_pitch;
    a.valid = valid; a.v_row = valid ? valid_row_pitch : 0; a.v_frame = valid ? valid_frame_pitch : 0;
    a.cameras = cameras; a.zbuf = (long long*)zbuf;
    a.frames = frames; a.h = h; a.w = w; a.H = H; a.W = W;
    const int64_t blocks = radius == 0 ? (n + kBlock - 1) / kBlock : (int64_t)ceil_div(h, kSrcTile) * ceil_div(w, kSrcTile);
    const dim3 grid((unsigned)(blocks < kSplatGridX ? blocks : kSplatGridX), (unsigned)(frames < kGridY ? frames : kGridY));
    if (radius == 0)      hipLaunchKernelGGL(view_splat_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
    else if (radius == 1) hipLaunchKernelGGL(view_splat_tiled_kernel<1>, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
    else                  hipLaunchKernelGGL(view_splat_tiled_kernel<2>, grid, dim3(kBlock), 0, (hipStream_t)stream, a);
    count_launch(FAM_AUX);
    return check_launch("view_splat");
}

extern "C" int p3d_view_resolve(const int64_t* zbuf, const uint8_t* src, int64_t src_row_pitch, int64_t src_frame_pitch, int32_t h, int32_t w,
                                int32_t channels, const uint8_t fill[4], uint8_t* dst, int64_t dst_row_pitch, int64_t dst_frame_pitch,
                                int32_t* index, uint8_t* status, const float* target_points, const float* cameras, int64_t tolerance,
                                int64_t* counts, int32_t frames, int32_t H, int32_t W, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(frames_ok(frames), "view_resolve: frames is 0 .. %d (got %d)", P3D_LABEL_MAX_FRAMES, frames);
    P3D_REQUIRE(view_size_ok(h, w) && view_size_ok(H, W), "view_resolve: a view is 1 .. %d pixels a side (got %d x %d into %d x %d)",
                P3D_PAINT_MAX_SIZE, h, w, H, W);
    P3D_REQUIRE(channels >= 1 && channels <= P3D_VIEW_MAX_CHANNELS, "view_resolve: channels is 1 .. 4 (got %d)", channels);
    if (frames == 0) return P3D_OK;
    P3D_REQUIRE(zbuf && src && fill && dst && status, "view_resolve: zbuf, src, fill, dst and status must be non-null");
    P3D_REQUIRE(pitches_ok(src_row_pitch, src_frame_pitch, h, (int64_t)w * channels, frames, true), "view_resolve: a pitch of src is shorter than its row or frame");
    P3D_REQUIRE(pitches_ok(dst_row_pitch, frames > 1 ? dst_frame_pitch : 1, H, (int64_t)W * channels, frames, false),
                "view_resolve: a pitch of dst is shorter than its row or frame");
    P3D_REQUIRE(!target_points || (cameras && tolerance >= 0 && tolerance <= P3D_VIEW_MAX_TOLERANCE),
                "view_resolve: target_points need cameras and a tolerance of 0 .. 2^31 - 1");
    P3D_REQUIRE(((uintptr_t)zbuf & 7u) == 0 && ((uintptr_t)index & 3u) == 0 && ((uintptr_t)counts & 7u) == 0 && ((uintptr_t)target_points & 3u) == 0 &&
                ((uintptr_t)cameras & 3u) == 0, "view_resolve: zbuf and counts must be 8-byte, index, target_points and cameras 4-byte aligned");
    const int64_t s_frames = src_frame_pitch == 0 ? 1 : frames;
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)((s_frames - 1) * src_frame_pitch + (int64_t)(h - 1) * src_row_pitch + (int64_t)w * channels);
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)((frames > 1 ? (frames - 1) * dst_frame_pitch : 0) + (int64_t)(H - 1) * dst_row_pitch + (int64_t)W * channels);
    P3D_REQUIRE(s1 <= d0 || d1 <= s0, "view_resolve: the frames are written out of place (src and dst overlap)");
    ResolveArgs a;
    a.zbuf = (const long long*)zbuf;
    a.src = src; a.s_row = src_row_pitch; a.s_frame = src_frame_pitch;
    a.dst = dst; a.d_row = dst_row_pitch; a.d_frame = frames > 1 ? dst_frame_pitch : 0;
    a.index = index; a.status = status; a.target = target_points; a.cameras = cameras; a.tolerance = tolerance;
    a.counts = (unsigned long long*)counts;
    a.fill = 0u;
    for (int c = 0; c < channels; ++c) a.fill |= (unsigned)fill[c] << (8 * c);
    a.frames = frames; a.n = h * w; a.w = w; a.C = channels; a.H = H; a.W = W;
    hipLaunchKernelGGL(view_resolve_kernel, view_grid((int64_t)H * W, frames, kGridX), dim3(kBlock), 0, (hipStream_t)stream, a);
    count_launch(FAM_AUX);
    return check_launch("view_resolve");
}

extern "C" int p3d_view_difference_histogram(const uint8_t* a, int64_t a_row_pitch, int64_t a_frame_pitch, const uint8_t* b, int64_t b_row_pitch,
                                             int64_t b_frame_pitch, const uint8_t* where, int64_t where_row_pitch, int64_t where_frame_pitch,
                                             int32_t match, int32_t channels, int32_t frames, int32_t H, int32_t W, int64_t* hist,
                                             p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(frames_ok(frames), "view_difference_histogram: frames is 0 .. %d (got %d)", P3D_LABEL_MAX_FRAMES, frames);
    P3D_REQUIRE(view_size_ok(H, W), "view_difference_histogram: a view is 1 .. %d pixels a side (got %d x %d)", P3D_PAINT_MAX_SIZE, H, W);
    P3D_REQUIRE(channels >= 1 && channels <= P3D_VIEW_MAX_CHANNELS, "view_difference_histogram: channels is 1 .. 4 (got %d)", channels);
    P3D_REQUIRE(match >= 0 && match <= 255, "view_difference_histogram: match is 0 .. 255 (got %d)", match);
    if (frames == 0) return P3D_OK;
    P3D_REQUIRE(a && b && hist, "view_difference_histogram: a, b and hist must be non-null");
    const int64_t bytes = (int64_t)W * channels;
    P3D_REQUIRE(pitches_ok(a_row_pitch, frames > 1 ? a_frame_pitch : 1, H, bytes, frames, false) &&
                pitches_ok(b_row_pitch, frames > 1 ? b_frame_pitch : 1, H, bytes, frames, false) &&
                (!where || pitches_ok(where_row_pitch, frames > 1 ? where_frame_pitch : 1, H, W, frames, false)),
                "view_difference_histogram: a pitch is shorter than its row or frame");
    P3D_REQUIRE(((uintptr_t)hist & 7u) == 0, "view_difference_histogram: hist must be 8-byte aligned");
    DiffArgs g;
    g.a = a; g.a_row = a_row_pitch; g.a_frame = frames > 1 ? a_frame_pitch : 0;
    g.b = b; g.b_row = b_row_pitch; g.b_frame = frames > 1 ? b_frame_pitch : 0;
    g.where = where; g.w_row = where ? where_row_pitch : 0; g.w_frame = (where && frames > 1) ? where_frame_pitch : 0;
    g.hist = (unsigned long long*)hist; g.frames = frames; g.C = channels; g.H = H; g.W = W; g.match = match;
    hipLaunchKernelGGL(view_difference_histogram_kernel, view_grid((int64_t)H * W, frames, kGridX), dim3(kBlock), 0, (hipStream_t)stream, g);
    count_launch(FAM_AUX);
    return check_launch("view_difference_histogram");
}
