// Host side of every entry point whose kernels read the tri-plane features through a p3d_render_desc: the descriptor checks that make
// the kernels' 32-bit plane addressing safe, the RenderArgs fill, the density kernels' persistent grid and the launch of kernels that
// need the per-device LDS opt-in.  shape.hip, surface.hip and render_bwd.hip call these.
// render.hip keeps its file-local check_render_common + fill_args (the committed counter passes pin its bytes): the next re-recording deletes the two and calls these.
#pragma once
#include "render_device.h"

namespace p3d {

// What gather_features / gather_features_coop rely on, in render.hip's order and with its messages behind `who`.  shared_ok: the entry
// point honours P3D_RENDER_SHARED_PLANES, so the span is one set's; set_rows: it launches one grid row per set (gridDim.y <= 65535).
inline int check_plane_desc(const p3d_render_desc* d, const char* who, bool shared_ok, bool set_rows = false)
{
    P3D_REQUIRE(d, "%s: null descriptor", who);
    P3D_REQUIRE(d->n_nets == 1 || d->n_nets == 2, "%s: n_nets must be 1 or 2 (got %d)", who, d->n_nets);
    P3D_REQUIRE(d->plane_h >= 1 && d->plane_w >= 1, "%s: bad plane size", who);
    P3D_REQUIRE(d->box_warp != 0.f, "%s: box_warp must be non-zero", who);
    P3D_REQUIRE(!set_rows || (d->n_img >= 0 && d->n_img <= 65535), "%s: n_img must be in [0, 65535] (got %d)", who, d->n_img);
    {   // 32-bit buffer addressing: the whole plane tensor must span < 2 GiB, a pixel stride < 64 KiB (24-bit multiplies for texel indices and strides)
        const int64_t istr = d->pixel_stride > 0 ? d->image_stride : (int64_t)3 * d->plane_h * d->plane_w * 32;
        const int64_t sets = (shared_ok && (d->raster_order & P3D_RENDER_SHARED_PLANES)) ? 1 : d->n_img;
        if (sets * istr * 4 >= ((int64_t)1 << 31) || (int64_t)d->plane_h * d->plane_w >= (1 << 24) || d->pixel_stride * 4 >= (1 << 16))
            return fail(P3D_ERR_UNSUPPORTED, "%s: plane tensor too large for 32-bit buffer addressing (%lld images)", who, (long long)d->n_img);
    }
    P3D_REQUIRE(d->pixel_stride == 0 || (d->pixel_stride % 4 == 0 && d->plane_stride % 4 == 0 && d->image_stride % 4 == 0),
                "%s: plane strides must keep texels 16-byte aligned", who);
    return P3D_OK;
}

// The plane fields of a checked descriptor: sizes, strides in floats and bytes, the bound of the buffer descriptor.
inline void fill_plane_args(RenderArgs& a, const p3d_render_desc* d, bool honour_shared)
{
    a.H = d->plane_h; a.W = d->plane_w; a.coord_scale = 2.f / d->box_warp;
    if (d->pixel_stride > 0) { a.plane_stride = d->plane_stride; a.pix_stride = d->pixel_stride; a.img_stride = d->image_stride; }
    else { a.plane_stride = (int64_t)a.H * a.W * 32; a.pix_stride = 32; a.img_stride = 3 * a.plane_stride; }
    a.plane_bytes = (unsigned)(a.plane_stride * 4); a.pix_bytes = (unsigned)(a.pix_stride * 4); a.img_bytes = (unsigned)(a.img_stride * 4);
    a.planes_total_bytes = (unsigned)((int64_t)d->n_img * a.img_stride * 4);
    if (honour_shared && (d->raster_order & P3D_RENDER_SHARED_PLANES)) {      // one plane set for all n_img ray sets: a zero image stride, and the buffer bound is that one set's
        a.planes_total_bytes = a.img_bytes; a.img_bytes = 0; a.img_stride = 0;
    }
}

// The ray-marching fields (n_img * rays_per_img fits an int: the entry points check it).
inline void fill_ray_args(RenderArgs& a, const p3d_render_desc* d)
{
    a.Sc = d->depth_resolution; a.Sf = d->depth_resolution_importance;
    a.ray_start = d->ray_start; a.ray_end = d->ray_end;
    a.lin_step = a.Sc > 1 ? (d->ray_end - d->ray_start) / (float)(a.Sc - 1) : 0.f;
    a.disparity = d->disparity_space_sampling; a.white_back = d->white_back; a.sem_sigmoid = d->semantic_sigmoid;
    a.total_rays = (int)((int64_t)d->n_img * d->rays_per_img); a.rays_per_img = d->rays_per_img;
    { int r = 1; while (r * r < d->rays_per_img) ++r; a.res = (r * r == d->rays_per_img && d->raster_order) ? r : 0; }
}

// The density kernels' persistent grid: tiles of 32 points, kWavesPerBlock tiles per block, about two blocks per CU over the whole
// launch, one grid row per set (n_sets >= 1).
inline dim3 set_row_grid(int64_t per_set, int n_sets)
{
    const int64_t tiles = (per_set + 31) / 32, cap = (kNumCU * 2 + n_sets - 1) / n_sets;
    const int64_t bx = (tiles + kWavesPerBlock - 1) / kWavesPerBlock;
    return dim3((unsigned)(bx < cap ? bx : cap), (unsigned)n_sets);
}

// Launch of a kernel that needs the opt-in to more than 64 KB of dynamic LDS.  The kernel is a template argument, so every kernel has
// its own per-device "already reserved" bits.  P3D_OK: enqueued (the caller checks the launch).
template <auto Kernel, class... Args>
inline int launch_lds_opt_in(const char* who, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, const Args&... args)
{
    static std::atomic<uint64_t> reserved_devs{0};
    const hipError_t e = reserve_lds_once((const void*)Kernel, (int)lds_bytes, reserved_devs);
    if (e != hipSuccess) return fail(P3D_ERR_LAUNCH, "%s: cannot reserve %zu B of LDS: %s", who, lds_bytes, hipGetErrorString(e));
    hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, s, args...);
    return P3D_OK;
}

} // namespace p3d
