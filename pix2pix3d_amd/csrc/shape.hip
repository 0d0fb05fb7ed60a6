// Shape extraction for gfx950: the density lattice and marching cubes (applications/extract_mesh.py:60-99).
//
// p3d_sample_lattice: the density of every point (xs[i], ys[j], zs[k]) of a regular lattice, N images, one launch.  The point
// query kernel (render.hip, sample_points_kernel) with what a density field does not need taken out: the coordinates come from three
// axis tables instead of 12 bytes per point, and only the density net runs (layer 1 + the sigma row of net n_nets - 1) — no colour
// net, no layer 2, no rgb stores.  The gather and the MLP pieces are render_device.h's, fed the same fp32 values in the same order,
// so a lattice density equals p3d_sample_points' density at the same point bit for bit.
//
// p3d_marching_cubes_classify / _emit: the triangle mesh of {u > threshold}, deterministic (no atomics; the output is a pure function
// of u and the threshold).  classify: per corner the edge mask and per cube the case, per 256-corner block the vertex and triangle
// totals.  The caller scans the block totals (exclusive) and allocates the outputs from the grand totals.  emit: two launches that
// redo the in-block scan (wave scan + LDS): the first writes the vertices and each corner's first vertex id, the second the faces,
// whose vertices belong to corners of other blocks as well.
#include "density_device.h"
#include "render_host.h"
#include "mc_tables.h"

namespace p3d {

// ---- density lattice ------------------------------------------------------------------------------------
template <int NNETS>
__global__ void __launch_bounds__(kWavesPerBlock * 64, 2)
lattice_sigma_kernel(RenderArgs a, const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs,
                     unsigned ny, unsigned nz, unsigned pts_per_img, float* __restrict__ sigma_out)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    stage_decoder(lds, a.decoder);
    __syncthreads();
    const rsrc_t rsrc = plane_rsrc(a);
    const unsigned img = blockIdx.y;                                 // one image per grid row: the in-image index stays 32-bit
    const unsigned img_off = img * a.img_bytes;
    float* out = sigma_out + (size_t)img * pts_per_img;
    const unsigned tiles = (pts_per_img + 31) / 32, nyz = ny * nz;
    for (unsigned t = blockIdx.x * kWavesPerBlock + wave; t < tiles; t += gridDim.x * kWavesPerBlock) {
        const unsigned q = tile_point(t, j, 0, 1);
        const bool live = q < pts_per_img;
        const unsigned p = live ? q : pts_per_img - 1;
        const unsigned ix = p / nyz, r = p - ix * nyz, iy = r / nz, iz = r - iy * nz;
        const float s = sigma_at<NNETS - 1>(a, rsrc, img_off, lds, lane, h, xs[ix], ys[iy], zs[iz]);
        if (live && h == 0) out[p] = s;
    }
}

// ---- marching cubes ---------------------------------------------------------------------------------------
constexpr int kMcBlock = 256;                    // corners per block (4 waves); the unit of the host-side scan

struct McGrid {
    const float* u; int64_t n;                   // n = X*Y*Z corners, row-major [X][Y][Z]
    int64_t yz; int32_t X, Y, Z; float thr;
};

__device__ __forceinline__ void mc_corner(const McGrid& g, int64_t c, int& i, int& j, int& k)
{
    i = (int)(c / g.yz);
    const int64_t r = c - (int64_t)i * g.yz;
    j = (int)(r / g.Z);
    k = (int)(r - (int64_t)j * g.Z);
}

// Inclusive sum over the 256 threads of the block (4 waves); `tot` gets the block total.  Every thread must call it.
__device__ __forceinline__ int block_inclusive_sum(int v, int* lds4, int& tot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int n = __shfl_up(v, o, 64);
        if (lane >= o) v += n;
    }
    if (lane == 63) lds4[wave] = v;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int w = 0; w < kMcBlock / 64; ++w) before += (w < wave) ? lds4[w] : 0;
    tot = lds4[0] + lds4[1] + lds4[2] + lds4[3];
    __syncthreads();                                                 // lds4 is reused by the next call
    return before + v;
}

__global__ void __launch_bounds__(kMcBlock) mc_classify_kernel(McGrid g, uint8_t* __restrict__ mask, uint8_t* __restrict__ cases,
                                                               int32_t* __restrict__ block_counts, int64_t n_blocks)
{
    __shared__ int lds4[4];
    const int64_t c = (int64_t)blockIdx.x * kMcBlock + threadIdx.x;
    int nv = 0, nf = 0;
    if (c < g.n) {
        int i, j, k;
        mc_corner(g, c, i, j, k);
        const float* u = g.u;
        const bool bx = i + 1 < g.X, by = j + 1 < g.Y, bz = k + 1 < g.Z;
        const bool in0 = u[c] > g.thr;
        const bool inx = bx && u[c + g.yz] > g.thr, iny = by && u[c + g.Z] > g.thr, inz = bz && u[c + 1] > g.thr;
        const unsigned m = (unsigned)(bx && inx != in0) | ((unsigned)(by && iny != in0) << 1) | ((unsigned)(bz && inz != in0) << 2);
        unsigned cs = 0;
        if (bx && by && bz) {
            const bool inxy = u[c + g.yz + g.Z] > g.thr, inxz = u[c + g.yz + 1] > g.thr, inyz = u[c + g.Z + 1] > g.thr;
            const bool inxyz = u[c + g.yz + g.Z + 1] > g.thr;
            cs = (unsigned)in0 | ((unsigned)inx << 1) | ((unsigned)iny << 2) | ((unsigned)inxy << 3)
               | ((unsigned)inz << 4) | ((unsigned)inxz << 5) | ((unsigned)inyz << 6) | ((unsigned)inxyz << 7);
        }
        mask[c] = (uint8_t)m;
        cases[c] = (uint8_t)cs;
        nv = __popc(m);
        nf = kMcTriCount[cs];
    }
    int tv, tf;
    block_inclusive_sum(nv, lds4, tv);
    block_inclusive_sum(nf, lds4, tf);
    if (threadIdx.x == 0) { block_counts[blockIdx.x] = tv; block_counts[n_blocks + blockIdx.x] = tf; }
}

__global__ void __launch_bounds__(kMcBlock) mc_vertices_kernel(McGrid g, const uint8_t* __restrict__ mask, const int64_t* __restrict__ block_voff,
                                                               int32_t* __restrict__ vbase, float* __restrict__ vertices)
{
    __shared__ int lds4[4];
    const int64_t c = (int64_t)blockIdx.x * kMcBlock + threadIdx.x;
    const unsigned m = (c < g.n) ? mask[c] : 0u;
    int tot;
    const int nv = __popc(m);
    const int64_t v0 = block_voff[blockIdx.x] + block_inclusive_sum(nv, lds4, tot) - nv;
    if (m == 0) return;
    vbase[c] = (int32_t)v0;
    int i, j, k;
    mc_corner(g, c, i, j, k);
    const float u0 = g.u[c];
    const int64_t step[3] = {g.yz, (int64_t)g.Z, 1};
    int64_t v = v0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!((m >> a) & 1u)) continue;
        const float t = (g.thr - u0) / (g.u[c + step[a]] - u0);
        float* dst = vertices + v * 3;
        dst[0] = (float)i + (a == 0 ? t : 0.f);
        dst[1] = (float)j + (a == 1 ? t : 0.f);
        dst[2] = (float)k + (a == 2 ? t : 0.f);
        ++v;
    }
}

__global__ void __launch_bounds__(kMcBlock) mc_faces_kernel(McGrid g, const uint8_t* __restrict__ mask, const uint8_t* __restrict__ cases,
                                                            const int64_t* __restrict__ block_foff, const int32_t* __restrict__ vbase,
                                                            int64_t* __restrict__ faces)
{
    __shared__ int lds4[4];
    const int64_t c = (int64_t)blockIdx.x * kMcBlock + threadIdx.x;
    const unsigned cs = (c < g.n) ? cases[c] : 0u;
    const int nf = kMcTriCount[cs];
    int tot;
    const int64_t f0 = block_foff[blockIdx.x] + block_inclusive_sum(nf, lds4, tot) - nf;
    if (nf == 0) return;
    const int64_t corner_off[8] = {0, g.yz, g.Z, g.yz + g.Z, 1, g.yz + 1, g.Z + 1, g.yz + g.Z + 1};
    int64_t* dst = faces + f0 * 3;
    for (int t = 0; t < nf * 3; ++t) {
        const int e = kMcTris[cs][t];
        const int64_t cc = c + corner_off[kMcEdgeCorner[e]];
        const unsigned a = (unsigned)kMcEdgeAxis[e];
        dst[t] = (int64_t)vbase[cc] + __popc((unsigned)mask[cc] & ((1u << a) - 1u));
    }
}

static int mc_check_dims(int32_t X, int32_t Y, int32_t Z, const char* what)
{
    P3D_REQUIRE(X >= 2 && Y >= 2 && Z >= 2, "%s: every dimension of the field must be >= 2 (got %d x %d x %d)", what, X, Y, Z);
    return P3D_OK;
}

} // namespace p3d

using namespace p3d;

extern "C" int p3d_sample_lattice(const float* planes_cl, const float* decoder, const p3d_render_desc* d, const float* xs, const float* ys,
                                  const float* zs, int32_t nx, int32_t ny, int32_t nz, float* sigma, p3d_stream_t stream)
{
    int rc = check_plane_desc(d, "sample_lattice", false, true);
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(planes_cl && decoder && xs && ys && zs && sigma, "sample_lattice: null pointer");
    P3D_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "sample_lattice: bad lattice size %d x %d x %d", nx, ny, nz);
    const int64_t per_img = (int64_t)nx * ny * nz;
    if (per_img > (int64_t)UINT32_MAX - 31)
        return fail(P3D_ERR_UNSUPPORTED, "sample_lattice: %lld points per image do not fit the kernel's 32-bit in-image index", (long long)per_img);
    if (d->n_img == 0) return P3D_OK;
    RenderArgs a{};
    fill_plane_args(a, d, false);
    a.planes = planes_cl; a.decoder = decoder;
    const size_t lds_bytes = (size_t)kDecoderFloats * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid = set_row_grid(per_img, d->n_img);
    if (d->n_nets == 1) hipLaunchKernelGGL(lattice_sigma_kernel<1>, grid, dim3(kWavesPerBlock * 64), lds_bytes, s, a, xs, ys, zs, (unsigned)ny, (unsigned)nz, (unsigned)per_img, sigma);
    else                hipLaunchKernelGGL(lattice_sigma_kernel<2>, grid, dim3(kWavesPerBlock * 64), lds_bytes, s, a, xs, ys, zs, (unsigned)ny, (unsigned)nz, (unsigned)per_img, sigma);
    count_launch(FAM_RENDER);
    return check_launch("sample_lattice");
}

extern "C" int64_t p3d_marching_cubes_blocks(int32_t X, int32_t Y, int32_t Z)
{
    if (X < 2 || Y < 2 || Z < 2) return 0;
    return ((int64_t)X * Y * Z + kMcBlock - 1) / kMcBlock;
}

extern "C" int p3d_marching_cubes_classify(const float* u, int32_t X, int32_t Y, int32_t Z, float threshold, uint8_t* mask, uint8_t* cases,
                                           int32_t* block_counts, p3d_stream_t stream)
{
    int rc = mc_check_dims(X, Y, Z, "marching_cubes_classify");
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(u && mask && cases && block_counts, "marching_cubes_classify: null pointer");
    const int64_t blocks = p3d_marching_cubes_blocks(X, Y, Z);
    if (blocks * kMcBlock > (int64_t)UINT32_MAX)                     // one thread per corner: the grid's work-items must fit 32 bits
        return fail(P3D_ERR_UNSUPPORTED, "marching_cubes_classify: field too large (%lld corners)", (long long)X * Y * Z);
    const McGrid g{u, (int64_t)X * Y * Z, (int64_t)Y * Z, X, Y, Z, threshold};
    hipLaunchKernelGGL(mc_classify_kernel, dim3((unsigned)blocks), dim3(kMcBlock), 0, (hipStream_t)stream, g, mask, cases, block_counts, blocks);
    count_launch(FAM_AUX);
    return check_launch("marching_cubes_classify");
}

extern "C" int p3d_marching_cubes_emit(const float* u, int32_t X, int32_t Y, int32_t Z, float threshold, const uint8_t* mask, const uint8_t* cases,
                                       const int64_t* block_voff, const int64_t* block_foff, int64_t n_vertices, int64_t n_faces,
                                       int32_t* vbase, float* vertices, int64_t* faces, p3d_stream_t stream)
{
    int rc = mc_check_dims(X, Y, Z, "marching_cubes_emit");
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(u && mask && cases && block_voff && block_foff && vbase, "marching_cubes_emit: null pointer");
    P3D_REQUIRE(n_vertices >= 0 && n_faces >= 0 && (n_vertices == 0 || vertices) && (n_faces == 0 || faces), "marching_cubes_emit: bad outputs");
    if (n_vertices > INT32_MAX)
        return fail(P3D_ERR_UNSUPPORTED, "marching_cubes_emit: %lld vertices do not fit the kernel's 32-bit vertex ids", (long long)n_vertices);
    const int64_t blocks = p3d_marching_cubes_blocks(X, Y, Z);
    if (blocks * kMcBlock > (int64_t)UINT32_MAX)
        return fail(P3D_ERR_UNSUPPORTED, "marching_cubes_emit: field too large (%lld corners)", (long long)X * Y * Z);
    if (n_vertices == 0) return P3D_OK;                              // (no crossed edge: no cube has a triangle either)
    const McGrid g{u, (int64_t)X * Y * Z, (int64_t)Y * Z, X, Y, Z, threshold};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_vertices_kernel, dim3((unsigned)blocks), dim3(kMcBlock), 0, s, g, mask, block_voff, vbase, vertices);
    count_launch(FAM_AUX);
    rc = check_launch("marching_cubes_vertices");
    if (rc != P3D_OK || n_faces == 0) return rc;
    hipLaunchKernelGGL(mc_faces_kernel, dim3((unsigned)blocks), dim3(kMcBlock), 0, s, g, mask, cases, block_foff, vbase, faces);
    count_launch(FAM_AUX);
    return check_launch("marching_cubes_faces");
}
