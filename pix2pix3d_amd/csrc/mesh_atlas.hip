// Texture atlases for gfx950: the geometry of every texel of a per-triangle atlas, the assembly of baked texel colours into the
// texture image, and a shade that samples it (include/p3d_hip.h, "mesh atlas"; pix2pix3d_amd/atlas.py).  All arithmetic is fp64 with
// every product and sum rounded on its own, in the header's order, so the outputs equal the operation-by-operation CPU formulation
// of atlas.py: byte for byte for the texels, the image and the albedo, within the headlight term's one level for a shaded frame.
//
// p3d_mesh_atlas_texels: one thread per texel in cell-major order; three dependent gathers (face -> corner ids -> positions and
// normals), 28 bytes stored per texel.
// p3d_mesh_atlas_assemble: one thread per texel of the IMAGE, which looks up the atlas texel it shows (or the background): every byte
// of the texture is written exactly once, in row order.
// p3d_mesh_shade_textured: one thread per pixel, as p3d_mesh_shade (whose triangle setup, barycentrics and headlight term it shares:
// mesh_tri.h); the albedo is a bilinear lookup with 8-bit fixed-point weights, an exact integer over 65536.  A footprint row is two
// texels = 6 contiguous bytes at any byte offset, fetched as 4 + 2 bytes as in mesh_bake.hip; the clamps of the lookup keep the
// 2 x 2 footprint inside the face's own cell whatever the barycentrics are (NaN included), so no address leaves the image.
#include "mesh_tri.h"

namespace p3d {

constexpr int kAtlasBlock = 256;
constexpr int kAtlasMinSize = 16, kAtlasMaxSize = 8192, kAtlasMinCell = 4;
constexpr int kAtlasMaxDim = 2048;                                   // frames, as the rasterizer's

struct Atlas { int32_t size, cell, per_row, n_faces, n_cells; };

// ---- texel geometry ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kAtlasBlock) atlas_texels_kernel(const float* __restrict__ vertices, int32_t nv,
                                                                   const int32_t* __restrict__ faces, const float* __restrict__ normals,
                                                                   Atlas a, float* __restrict__ points, float* __restrict__ texel_normals,
                                                                   int32_t* __restrict__ face)
{
#pragma clang fp contract(off)
    const int64_t q = (int64_t)blockIdx.x * kAtlasBlock + threadIdx.x;
    const int32_t cc = a.cell * a.cell;
    if (q >= (int64_t)a.n_cells * cc) return;
    const int32_t k = (int32_t)(q / cc), rem = (int32_t)(q - (int64_t)k * cc);
    const int32_t j = rem / a.cell, i = rem - j * a.cell;
    const int32_t half = i + j > a.cell - 2 ? 1 : 0;
    const int32_t ip = half ? a.cell - 1 - i : i, jp = half ? a.cell - 1 - j : j;
    const int32_t m = a.cell - 3;
    const double n0 = (double)(m - ip - jp), n1 = (double)ip, n2 = (double)jp, md = (double)m;
    const int64_t t = 2 * (int64_t)k + half;
    int32_t idx[3] = {0, 0, 0};
    bool ok = t < a.n_faces;
    if (ok) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            idx[c] = faces[t * 3 + c];
            ok = ok && (unsigned)idx[c] < (unsigned)nv;
        }
    }
    face[q] = ok ? (int32_t)t : -1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float p = 0.0f, n = 0.0f;
        if (ok) {
            double s = n0 * (double)vertices[(int64_t)idx[0] * 3 + c];
            s = s + n1 * (double)vertices[(int64_t)idx[1] * 3 + c];
            s = s + n2 * (double)vertices[(int64_t)idx[2] * 3 + c];
            p = (float)(s / md);
            s = n0 * (double)normals[(int64_t)idx[0] * 3 + c];
            s = s + n1 * (double)normals[(int64_t)idx[1] * 3 + c];
            s = s + n2 * (double)normals[(int64_t)idx[2] * 3 + c];
            n = (float)(s / md);
        }
        points[q * 3 + c] = p;
        texel_normals[q * 3 + c] = n;
    }
}

// ---- assembly ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kAtlasBlock) atlas_assemble_kernel(const uint8_t* __restrict__ colors, const int32_t* __restrict__ face,
                                                                     Atlas a, int bg_r, int bg_g, int bg_b, uint8_t* __restrict__ texture)
{
    const int64_t o = (int64_t)blockIdx.x * kAtlasBlock + threadIdx.x;
    if (o >= (int64_t)a.size * a.size) return;
    const int32_t row = (int32_t)(o / a.size), col = (int32_t)(o - (int64_t)row * a.size);
    const int32_t cr = row / a.cell, ccol = col / a.cell;
    const int64_t k = (int64_t)cr * a.per_row + ccol;
    uint8_t r = (uint8_t)bg_r, g = (uint8_t)bg_g, b = (uint8_t)bg_b;
    if (ccol < a.per_row && k < a.n_cells) {
        const int64_t q = (k * a.cell + (row - cr * a.cell)) * a.cell + (col - ccol * a.cell);
        if (face[q] >= 0) { r = colors[q * 3]; g = colors[q * 3 + 1]; b = colors[q * 3 + 2]; }
    }
    texture[o * 3] = r; texture[o * 3 + 1] = g; texture[o * 3 + 2] = b;
}

// ---- textured shade: one thread per pixel ----------------------------------------------------------------------------------------
// rint(v * 256) clamped to [0, hi], as an integer; a NaN goes to 0.
__device__ __forceinline__ int32_t atlas_fixed(double v, int32_t hi)
{
#pragma clang fp contract(off)
    const double x = rint(v * 256.0);
    return x >= 0.0 ? (x > (double)hi ? hi : (int32_t)x) : 0;
}

__global__ void __launch_bounds__(kAtlasBlock) mesh_shade_textured_kernel(const int32_t* __restrict__ face_id, const int4* __restrict__ proj,
                                                                          const float* __restrict__ vertices, int nv,
                                                                          const int32_t* __restrict__ faces, const uint8_t* __restrict__ texture,
                                                                          Atlas a, const float* __restrict__ cameras, int n_frames, int ortho,
                                                                          int W, int H, float ambient, int bg_r, int bg_g, int bg_b,
                                                                          uint8_t* __restrict__ rgb)
{
#pragma clang fp contract(off)
    const int64_t hw = (int64_t)H * W, total = (int64_t)n_frames * hw;
    for (int64_t i = (int64_t)blockIdx.x * kAtlasBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kAtlasBlock) {
        const int f = (int)(i / hw);
        const int64_t p = i - (int64_t)f * hw;
        const int r = (int)(p / W), c = (int)(p - (int64_t)r * W);
        const int t = face_id[i];
        uint8_t* out = rgb + i * 3;
        Tri T;
        if (t < 0 || t >= a.n_faces || !tri_setup(proj + (int64_t)f * nv, faces, t, nv, W, H, T)) {
            out[0] = (uint8_t)bg_r; out[1] = (uint8_t)bg_g; out[2] = (uint8_t)bg_b;
            continue;
        }
        int64_t w[3];
        tri_weights(T, r, c, w[0], w[1], w[2]);
        double b[3];
        tri_barycentrics(T, w, ortho != 0, b);
        const double shade = tri_headlight(vertices, T.idx, cameras + (int64_t)f * kCamFloats, ambient);
        // back into the face's stored corner order (a drawn face has three different corners, so this tells a swap)
        const bool swapped = T.idx[1] != faces[(int64_t)t * 3 + 1];
        const double b1 = swapped ? b[2] : b[1], b2 = swapped ? b[1] : b[2];
        const int32_t k = t >> 1, top = a.cell - 1;
        const double md = (double)(a.cell - 3);
        double x = b1 * md, y = b2 * md;
        if (t & 1) { x = (double)top - x; y = (double)top - y; }
        const int32_t X = atlas_fixed(x, top * 256), Y = atlas_fixed(y, top * 256);
        const int32_t c0 = min(X >> 8, a.cell - 2), r0 = min(Y >> 8, a.cell - 2);
        const int32_t fx = X - (c0 << 8), fy = Y - (r0 << 8);
        const int64_t tap = ((int64_t)(k / a.per_row) * a.cell + r0) * a.size + (int64_t)(k % a.per_row) * a.cell + c0;
        uint32_t lo[2];
        uint16_t hi[2];
#pragma unroll
        for (int row = 0; row < 2; ++row) {
            const uint8_t* src = texture + (tap + (int64_t)row * a.size) * 3;
            __builtin_memcpy(&lo[row], src, 4);
            __builtin_memcpy(&hi[row], src + 4, 2);
        }
        const uint32_t t0[6] = {lo[0] & 255u, (lo[0] >> 8) & 255u, (lo[0] >> 16) & 255u, lo[0] >> 24, hi[0] & 255u, (uint32_t)hi[0] >> 8};
        const uint32_t t1[6] = {lo[1] & 255u, (lo[1] >> 8) & 255u, (lo[1] >> 16) & 255u, lo[1] >> 24, hi[1] & 255u, (uint32_t)hi[1] >> 8};
        const int32_t w00 = (256 - fy) * (256 - fx), w01 = (256 - fy) * fx, w10 = fy * (256 - fx), w11 = fy * fx;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int32_t num = w00 * (int32_t)t0[ch] + w01 * (int32_t)t0[3 + ch] + w10 * (int32_t)t1[ch] + w11 * (int32_t)t1[3 + ch];
            out[ch] = shaded_byte((double)num / 65536.0, shade);
        }
    }
}

// The layout's rules (atlas.layout): an error code, with the message set, when (n_faces, size, cell) is not what an atlas can have.
static int atlas_check(const char* what, int32_t n_faces, int32_t size, int32_t cell, Atlas& a)
{
    P3D_REQUIRE(n_faces >= 0, "%s: negative face count %d", what, n_faces);
    if (n_faces > INT32_MAX - 1) return fail(P3D_ERR_UNSUPPORTED, "%s: at most INT32_MAX - 1 faces (got %d)", what, n_faces);
    P3D_REQUIRE(size >= kAtlasMinSize && size <= kAtlasMaxSize, "%s: atlas size %d outside [%d, %d]", what, size, kAtlasMinSize, kAtlasMaxSize);
    P3D_REQUIRE(cell >= kAtlasMinCell && cell <= size, "%s: cell %d outside [%d, size = %d]", what, cell, kAtlasMinCell, size);
    a.size = size; a.cell = cell; a.per_row = size / cell; a.n_faces = n_faces; a.n_cells = (int32_t)(((int64_t)n_faces + 1) / 2);
    P3D_REQUIRE((int64_t)a.n_cells <= (int64_t)a.per_row * a.per_row, "%s: %d faces need %d cells, an atlas of %d^2 texels with cells of %d holds %d",
                what, n_faces, a.n_cells, size, cell, a.per_row * a.per_row);
    return P3D_OK;
}

static inline unsigned atlas_blocks(int64_t n) { return (unsigned)((n + kAtlasBlock - 1) / kAtlasBlock); }

} // namespace p3d

using namespace p3d;

extern "C" int p3d_mesh_atlas_texels(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces, const float* normals,
                                     int32_t size, int32_t cell, float* points, float* texel_normals, int32_t* face, p3d_stream_t stream)
{
    Atlas a;
    int rc = atlas_check("mesh_atlas_texels", n_faces, size, cell, a);
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(n_vertices >= 0, "mesh_atlas_texels: negative vertex count %d", n_vertices);
    if (n_vertices > INT32_MAX - 1) return fail(P3D_ERR_UNSUPPORTED, "mesh_atlas_texels: at most INT32_MAX - 1 vertices (got %d)", n_vertices);
    if (a.n_cells == 0) return P3D_OK;
    P3D_REQUIRE(faces && points && texel_normals && face && (n_vertices == 0 || (vertices && normals)), "mesh_atlas_texels: null pointer");
    hipLaunchKernelGGL(atlas_texels_kernel, dim3(atlas_blocks((int64_t)a.n_cells * cell * cell)), dim3(kAtlasBlock), 0, (hipStream_t)stream,
                       vertices, n_vertices, faces, normals, a, points, texel_normals, face);
    count_launch(FAM_AUX);
    return check_launch("mesh_atlas_texels");
}

extern "C" int p3d_mesh_atlas_assemble(const uint8_t* colors, const int32_t* face, int32_t n_faces, int32_t size, int32_t cell,
                                       int32_t bg_r, int32_t bg_g, int32_t bg_b, uint8_t* texture, p3d_stream_t stream)
{
    Atlas a;
    int rc = atlas_check("mesh_atlas_assemble", n_faces, size, cell, a);
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(texture && (a.n_cells == 0 || (colors && face)), "mesh_atlas_assemble: null pointer");
    hipLaunchKernelGGL(atlas_assemble_kernel, dim3(atlas_blocks((int64_t)size * size)), dim3(kAtlasBlock), 0, (hipStream_t)stream, colors, face,
                       a, bg_r & 255, bg_g & 255, bg_b & 255, texture);
    count_launch(FAM_AUX);
    return check_launch("mesh_atlas_assemble");
}

extern "C" int p3d_mesh_shade_textured(const int32_t* face_id, const int32_t* proj, const float* vertices, int32_t n_vertices,
                                       const int32_t* faces, int32_t n_faces, const uint8_t* texture, int32_t size, int32_t cell,
                                       const float* cameras, int32_t n_frames, int32_t orthographic, int32_t width, int32_t height,
                                       float ambient, int32_t bg_r, int32_t bg_g, int32_t bg_b, uint8_t* rgb, p3d_stream_t stream)
{
    Atlas a;
    int rc = atlas_check("mesh_shade_textured", n_faces, size, cell, a);
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(n_vertices >= 0 && n_vertices < INT32_MAX, "mesh_shade_textured: bad vertex count %d", n_vertices);
    P3D_REQUIRE(n_frames >= 0 && n_frames <= 65535, "mesh_shade_textured: n_frames must be in [0, 65535] (got %d)", n_frames);
    P3D_REQUIRE(width >= 1 && height >= 1 && width <= kAtlasMaxDim && height <= kAtlasMaxDim,
                "mesh_shade_textured: image size %d x %d outside [1, %d]^2", width, height, kAtlasMaxDim);
    if (n_frames == 0) return P3D_OK;
    P3D_REQUIRE(face_id && cameras && rgb && texture && (n_vertices == 0 || (proj && vertices)) && (n_faces == 0 || faces),
                "mesh_shade_textured: null pointer");
    int64_t g = ((int64_t)n_frames * width * height + kAtlasBlock - 1) / kAtlasBlock;
    g = g > kNumCU * 16 ? kNumCU * 16 : g;
    hipLaunchKernelGGL(mesh_shade_textured_kernel, dim3((unsigned)g), dim3(kAtlasBlock), 0, (hipStream_t)stream, face_id, (const int4*)proj,
                       vertices, n_vertices, faces, texture, a, cameras, n_frames, orthographic, width, height, ambient, bg_r & 255, bg_g & 255,
                       bg_b & 255, rgb);
    count_launch(FAM_AUX);
    return check_launch("mesh_shade_textured");
}
