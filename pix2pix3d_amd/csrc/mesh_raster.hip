// Mesh rendering for gfx950: projection, a screen-tiled triangle rasterizer and headlight shading (the role of pyrender in
// applications/extract_mesh.py:226-262).  Conventions (cameras, fixed point, fill rule, depth, z-test key): include/p3d_hip.h.
//
// p3d_mesh_project: one thread per (frame, vertex), fp64, one 16-byte record (sx, sy, z bits, dropped) per vertex and frame.
// p3d_mesh_raster_count / _bin: per frame, every triangle whose pixel-centre bounding box is not empty is listed in every screen tile
// that box meets.  A work-group first counts its triangles per tile in an LDS histogram, then makes one global atomic per non-empty
// tile (count: the add; bin: the reservation of a range of list slots, handed out again through LDS atomics).
// p3d_mesh_raster: one work-group per (tile, frame) rasterizes its list into an LDS z-buffer of 64-bit keys with LDS atomicMin, then
// stores the tile once.  Lane-scattered 8-byte global atomics to random pixels would run at the memory side, far below the chip's
// atomic rate; the LDS minimum needs none.  Each list entry is one thread, which walks the triangle's pixel centres inside the tile.
// p3d_mesh_shade: one thread per pixel.  Triangle setup, coverage, barycentrics and the headlight term live in mesh_tri.h, which the
// textured shade of mesh_atlas.hip shares.
#include "mesh_tri.h"

namespace p3d {

constexpr int kTile = P3D_MESH_TILE;
constexpr int kTileShift = 5;
static_assert((1 << kTileShift) == kTile, "tile edge");
constexpr int kMaxDim = 2048;
constexpr int kMaxTiles = (kMaxDim / kTile) * (kMaxDim / kTile);          // 4096: the LDS histogram of count / bin (16 KiB)
constexpr int kBlock = 256;
constexpr int64_t kGuard = 4096 * 256;                                    // guard band, in sub-pixel units

__device__ __forceinline__ float tri_depth(float z0, float z1, float z2, int64_t w0, int64_t w1, int64_t w2, bool ortho)
{
#pragma clang fp contract(off)
    const double a = (double)w0, b = (double)w1, c = (double)w2;
    double s = a + b;
    s = s + c;
    double d;
    if (ortho) {
        double n = a * (double)z0;
        n = n + b * (double)z1;
        n = n + c * (double)z2;
        d = n / s;
    } else {
        double q = a / (double)z0;
        q = q + b / (double)z1;
        q = q + c / (double)z2;
        d = s / q;
    }
    return (float)d;
}

// ---- projection ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) mesh_project_kernel(const float* __restrict__ vertices, int nv, const float* __restrict__ cameras,
                                                              int n_frames, int ortho, int W, int H, int4* __restrict__ proj)
{
#pragma clang fp contract(off)
    const int64_t total = (int64_t)n_frames * nv;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int f = (int)(i / nv);
        const int64_t v = i - (int64_t)f * nv;
        const float* cam = cameras + (int64_t)f * kCamFloats;
        const double px = (double)vertices[v * 3 + 0] - (double)cam[3];
        const double py = (double)vertices[v * 3 + 1] - (double)cam[7];
        const double pz = (double)vertices[v * 3 + 2] - (double)cam[11];
        double xc = (double)cam[0] * px; xc = xc + (double)cam[4] * py; xc = xc + (double)cam[8] * pz;
        double yc = (double)cam[1] * px; yc = yc + (double)cam[5] * py; yc = yc + (double)cam[9] * pz;
        double zc = (double)cam[2] * px; zc = zc + (double)cam[6] * py; zc = zc + (double)cam[10] * pz;
        double u, w;
        if (ortho) {
            u = (xc / (double)cam[16] + 1.0) * 0.5;
            w = (yc / (double)cam[17] + 1.0) * 0.5;
        } else {
            double a = (double)cam[16] * xc;
            a = a + (double)cam[20] * yc;
            u = a / zc + (double)cam[18];
            w = ((double)cam[17] * yc) / zc + (double)cam[19];
        }
        const double sx = u * (double)(W * 256), sy = w * (double)(H * 256);
        const bool keep = zc >= (double)cam[21] && zc <= (double)cam[22] &&
                          sx >= (double)-kGuard && sx <= (double)((int64_t)W * 256 + kGuard) &&
                          sy >= (double)-kGuard && sy <= (double)((int64_t)H * 256 + kGuard);
        int4 rec;
        rec.x = keep ? (int)rint(sx) : 0;
        rec.y = keep ? (int)rint(sy) : 0;
        rec.z = __float_as_int((float)zc);
        rec.w = keep ? 0 : 1;
        proj[i] = rec;
    }
}

// ---- binning ------------------------------------------------------------------------------------------------------------------
// BIN = false: tile_counts[f][tile] += triangles of this work-group meeting the tile.  BIN = true: reserve a range of the tile's list
// slots per work-group (cursor starts at the tile's offset), then write the triangle ids into it.
template <bool BIN>
__global__ void __launch_bounds__(kBlock) mesh_bin_kernel(const int4* __restrict__ proj, int nv, const int32_t* __restrict__ faces, int nf,
                                                          int W, int H, int tiles_x, int n_tiles, int32_t* __restrict__ tile_counts,
                                                          int64_t* __restrict__ tile_cursor, int32_t* __restrict__ tile_list)
{
    __shared__ int hist[kMaxTiles];
    __shared__ int64_t base[BIN ? kMaxTiles : 1];
    const int f = blockIdx.y;
    const int4* pf = proj + (int64_t)f * nv;
    for (int i = threadIdx.x; i < n_tiles; i += kBlock) hist[i] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < nf; t += stride) {
        Tri T;
        if (!tri_setup(pf, faces, t, nv, W, H, T)) continue;
        for (int ty = T.r0 >> kTileShift; ty <= (T.r1 >> kTileShift); ++ty)
            for (int tx = T.c0 >> kTileShift; tx <= (T.c1 >> kTileShift); ++tx) atomicAdd(&hist[ty * tiles_x + tx], 1);
    }
    __syncthreads();
    const int64_t row = (int64_t)f * n_tiles;
    for (int i = threadIdx.x; i < n_tiles; i += kBlock) {
        const int n = hist[i];
        if (n == 0) continue;
        if (BIN) {
            base[i] = (int64_t)atomicAdd((unsigned long long*)&tile_cursor[row + i], (unsigned long long)n);
            hist[i] = 0;
        } else {
            atomicAdd(&tile_counts[row + i], n);
        }
    }
    if (!BIN) return;
    __syncthreads();
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < nf; t += stride) {
        Tri T;
        if (!tri_setup(pf, faces, t, nv, W, H, T)) continue;
        for (int ty = T.r0 >> kTileShift; ty <= (T.r1 >> kTileShift); ++ty)
            for (int tx = T.c0 >> kTileShift; tx <= (T.c1 >> kTileShift); ++tx) {
                const int i = ty * tiles_x + tx;
                tile_list[base[i] + atomicAdd(&hist[i], 1)] = (int32_t)t;
            }
    }
}

// ---- rasterization: one work-group per (tile, frame) ----------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) mesh_raster_kernel(const int4* __restrict__ proj, int nv, const int32_t* __restrict__ faces,
                                                             int W, int H, int tiles_x, int n_tiles, int ortho,
                                                             const int32_t* __restrict__ tile_counts, const int64_t* __restrict__ tile_offsets,
                                                             const int32_t* __restrict__ tile_list, int32_t* __restrict__ face_id,
                                                             float* __restrict__ depth)
{
    __shared__ unsigned long long zbuf[kTile * kTile];
    const int tile = blockIdx.x, f = blockIdx.y;
    const int tr0 = (tile / tiles_x) * kTile, tc0 = (tile % tiles_x) * kTile;
    const int4* pf = proj + (int64_t)f * nv;
    for (int i = threadIdx.x; i < kTile * kTile; i += kBlock) zbuf[i] = ~0ull;
    __syncthreads();
    const int64_t k = (int64_t)f * n_tiles + tile;
    const int n = tile_counts[k];
    const int32_t* list = tile_list + tile_offsets[k];
    for (int e = threadIdx.x; e < n; e += kBlock) {
        const int t = list[e];
        Tri T;
        if (!tri_setup(pf, faces, t, nv, W, H, T)) continue;          // (binned, so always drawn)
        const int r0 = max(T.r0, tr0), r1 = min(T.r1, tr0 + kTile - 1);
        const int c0 = max(T.c0, tc0), c1 = min(T.c1, tc0 + kTile - 1);
        for (int r = r0; r <= r1; ++r)
            for (int c = c0; c <= c1; ++c) {
                int64_t w0, w1, w2;
                if (!tri_weights(T, r, c, w0, w1, w2)) continue;
                const float d = tri_depth(T.z[0], T.z[1], T.z[2], w0, w1, w2, ortho != 0);
                const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)t;
                atomicMin(&zbuf[(r - tr0) * kTile + (c - tc0)], key);
            }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTile * kTile; i += kBlock) {
        const int r = tr0 + (i >> kTileShift), c = tc0 + (i & (kTile - 1));
        if (r >= H || c >= W) continue;
        const unsigned long long key = zbuf[i];
        const int64_t o = ((int64_t)f * H + r) * W + c;
        face_id[o] = key == ~0ull ? -1 : (int32_t)(unsigned)(key & 0xffffffffull);
        depth[o] = key == ~0ull ? __int_as_float(0x7f800000) : __uint_as_float((unsigned)(key >> 32));
    }
}

// ---- shading: one thread per pixel ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) mesh_shade_kernel(const int32_t* __restrict__ face_id, const int4* __restrict__ proj,
                                                            const float* __restrict__ vertices, int nv, const int32_t* __restrict__ faces, int nf,
                                                            const uint8_t* __restrict__ colors, const float* __restrict__ cameras, int n_frames,
                                                            int ortho, int W, int H, float ambient, int bg_r, int bg_g, int bg_b,
                                                            uint8_t* __restrict__ rgb)
{
#pragma clang fp contract(off)
    const int64_t hw = (int64_t)H * W, total = (int64_t)n_frames * hw;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int f = (int)(i / hw);
        const int64_t p = i - (int64_t)f * hw;
        const int r = (int)(p / W), c = (int)(p - (int64_t)r * W);
        const int t = face_id[i];
        uint8_t* out = rgb + i * 3;
        Tri T;
        if (t < 0 || t >= nf || !tri_setup(proj + (int64_t)f * nv, faces, t, nv, W, H, T)) {
            out[0] = (uint8_t)bg_r; out[1] = (uint8_t)bg_g; out[2] = (uint8_t)bg_b;
            continue;
        }
        int64_t w[3];
        tri_weights(T, r, c, w[0], w[1], w[2]);
        const int* idx = T.idx;
        double b[3];
        tri_barycentrics(T, w, ortho != 0, b);
        const double shade = tri_headlight(vertices, idx, cameras + (int64_t)f * kCamFloats, ambient);
        for (int ch = 0; ch < 3; ++ch) {
            double a;
            if (colors) {
                a = b[0] * (double)colors[(int64_t)idx[0] * 3 + ch];
                a = a + b[1] * (double)colors[(int64_t)idx[1] * 3 + ch];
                a = a + b[2] * (double)colors[(int64_t)idx[2] * 3 + ch];
            } else {
                a = (double)P3D_MESH_GREY;
            }
            out[ch] = shaded_byte(a, shade);
        }
    }
}

static int mesh_check(int32_t nv, int32_t n_frames, int32_t W, int32_t H, const char* what)
{
    P3D_REQUIRE(nv >= 0 && nv < INT32_MAX, "%s: bad vertex count %d", what, nv);
    P3D_REQUIRE(n_frames >= 0 && n_frames <= 65535, "%s: n_frames must be in [0, 65535] (got %d)", what, n_frames);
    P3D_REQUIRE(W >= 1 && H >= 1 && W <= kMaxDim && H <= kMaxDim, "%s: image size %d x %d outside [1, %d]^2", what, W, H, kMaxDim);
    return P3D_OK;
}

static unsigned grid_for(int64_t work, int64_t cap)
{
    int64_t g = (work + kBlock - 1) / kBlock;
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

} // namespace p3d

using namespace p3d;

extern "C" int p3d_mesh_project(const float* vertices, int32_t n_vertices, const float* cameras, int32_t n_frames, int32_t orthographic,
                                int32_t width, int32_t height, int32_t* proj, p3d_stream_t stream)
{
    int rc = mesh_check(n_vertices, n_frames, width, height, "mesh_project");
    if (rc != P3D_OK) return rc;
    if (n_vertices == 0 || n_frames == 0) return P3D_OK;
    P3D_REQUIRE(vertices && cameras && proj, "mesh_project: null pointer");
    hipLaunchKernelGGL(mesh_project_kernel, dim3(grid_for((int64_t)n_frames * n_vertices, kNumCU * 16)), dim3(kBlock), 0, (hipStream_t)stream,
                       vertices, n_vertices, cameras, n_frames, orthographic, width, height, (int4*)proj);
    count_launch(FAM_AUX);
    return check_launch("mesh_project");
}

extern "C" int32_t p3d_mesh_raster_tiles(int32_t width, int32_t height)
{
    if (width < 1 || height < 1) return 0;
    return ((width + kTile - 1) / kTile) * ((height + kTile - 1) / kTile);
}

static int mesh_bin_launch(bool bin, const int32_t* proj, int32_t nv, const int32_t* faces, int32_t nf, int32_t n_frames, int32_t W, int32_t H,
                           int32_t* tile_counts, int64_t* tile_cursor, int32_t* tile_list, hipStream_t s)
{
    const int tiles_x = (W + kTile - 1) / kTile, n_tiles = p3d_mesh_raster_tiles(W, H);
    // about 2048 work-groups over the whole launch: each makes at most n_tiles global atomics
    const unsigned gx = grid_for(nf, (2048 + n_frames - 1) / n_frames);
    const dim3 grid(gx, (unsigned)n_frames);
    if (bin) hipLaunchKernelGGL(mesh_bin_kernel<true>, grid, dim3(kBlock), 0, s, (const int4*)proj, nv, faces, nf, W, H, tiles_x, n_tiles,
                                tile_counts, tile_cursor, tile_list);
    else     hipLaunchKernelGGL(mesh_bin_kernel<false>, grid, dim3(kBlock), 0, s, (const int4*)proj, nv, faces, nf, W, H, tiles_x, n_tiles,
                                tile_counts, tile_cursor, tile_list);
    count_launch(FAM_AUX);
    return check_launch(bin ? "mesh_raster_bin" : "mesh_raster_count");
}

extern "C" int p3d_mesh_raster_count(const int32_t* proj, int32_t n_vertices, const int32_t* faces, int32_t n_faces, int32_t n_frames,
                                     int32_t width, int32_t height, int32_t* tile_counts, p3d_stream_t stream)
{
    int rc = mesh_check(n_vertices, n_frames, width, height, "mesh_raster_count");
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(n_faces >= 0 && n_faces < INT32_MAX, "mesh_raster_count: bad face count %d", n_faces);
    if (n_frames == 0) return P3D_OK;
    P3D_REQUIRE(tile_counts, "mesh_raster_count: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(tile_counts, 0, sizeof(int32_t) * (size_t)n_frames * p3d_mesh_raster_tiles(width, height), s) != hipSuccess)
        return fail(P3D_ERR_LAUNCH, "mesh_raster_count: memset failed");
    if (n_faces == 0 || n_vertices == 0) return P3D_OK;
    P3D_REQUIRE(proj && faces, "mesh_raster_count: null pointer");
    return mesh_bin_launch(false, proj, n_vertices, faces, n_faces, n_frames, width, height, tile_counts, nullptr, nullptr, s);
}

extern "C" int p3d_mesh_raster_bin(const int32_t* proj, int32_t n_vertices, const int32_t* faces, int32_t n_faces, int32_t n_frames,
                                   int32_t width, int32_t height, const int64_t* tile_offsets, int64_t* tile_cursor, int32_t* tile_list,
                                   p3d_stream_t stream)
{
    int rc = mesh_check(n_vertices, n_frames, width, height, "mesh_raster_bin");
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(n_faces >= 0 && n_faces < INT32_MAX, "mesh_raster_bin: bad face count %d", n_faces);
    if (n_frames == 0 || n_faces == 0 || n_vertices == 0) return P3D_OK;
    P3D_REQUIRE(proj && faces && tile_offsets && tile_cursor, "mesh_raster_bin: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(tile_cursor, tile_offsets, sizeof(int64_t) * (size_t)n_frames * p3d_mesh_raster_tiles(width, height),
                       hipMemcpyDeviceToDevice, s) != hipSuccess)
        return fail(P3D_ERR_LAUNCH, "mesh_raster_bin: cursor copy failed");
    return mesh_bin_launch(true, proj, n_vertices, faces, n_faces, n_frames, width, height, nullptr, tile_cursor, tile_list, s);
}

extern "C" int p3d_mesh_raster(const int32_t* proj, int32_t n_vertices, const int32_t* faces, int32_t n_frames, int32_t width, int32_t height,
                               int32_t orthographic, const int32_t* tile_counts, const int64_t* tile_offsets, const int32_t* tile_list,
                               int32_t* face_id, float* depth, p3d_stream_t stream)
{
    int rc = mesh_check(n_vertices, n_frames, width, height, "mesh_raster");
    if (rc != P3D_OK) return rc;
    if (n_frames == 0) return P3D_OK;
    P3D_REQUIRE(tile_counts && tile_offsets && face_id && depth, "mesh_raster: null pointer");
    const int tiles_x = (width + kTile - 1) / kTile, n_tiles = p3d_mesh_raster_tiles(width, height);
    hipLaunchKernelGGL(mesh_raster_kernel, dim3((unsigned)n_tiles, (unsigned)n_frames), dim3(kBlock), 0, (hipStream_t)stream,
                       (const int4*)proj, n_vertices, faces, width, height, tiles_x, n_tiles, orthographic, tile_counts, tile_offsets,
                       tile_list, face_id, depth);
    count_launch(FAM_AUX);
    return check_launch("mesh_raster");
}

extern "C" int p3d_mesh_shade(const int32_t* face_id, const int32_t* proj, const float* vertices, int32_t n_vertices, const int32_t* faces,
                              int32_t n_faces, const uint8_t* colors, const float* cameras, int32_t n_frames, int32_t orthographic,
                              int32_t width, int32_t height, float ambient, int32_t bg_r, int32_t bg_g, int32_t bg_b, uint8_t* rgb,
                              p3d_stream_t stream)
{
    int rc = mesh_check(n_vertices, n_frames, width, height, "mesh_shade");
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(n_faces >= 0 && n_faces < INT32_MAX, "mesh_shade: bad face count %d", n_faces);
    if (n_frames == 0) return P3D_OK;
    P3D_REQUIRE(face_id && cameras && rgb && (n_vertices == 0 || (proj && vertices)) && (n_faces == 0 || faces), "mesh_shade: null pointer");
    hipLaunchKernelGGL(mesh_shade_kernel, dim3(grid_for((int64_t)n_frames * width * height, kNumCU * 16)), dim3(kBlock), 0, (hipStream_t)stream,
                       face_id, (const int4*)proj, vertices, n_vertices, faces, n_faces, colors, cameras, n_frames, orthographic, width, height,
                       ambient, bg_r & 255, bg_g & 255, bg_b & 255, rgb);
    count_launch(FAM_AUX);
    return check_launch("mesh_shade");
}
