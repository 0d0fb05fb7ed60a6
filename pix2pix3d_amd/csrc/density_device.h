// Device-side pieces the density kernels share (shape.hip: lattice_sigma_kernel; surface.hip: surface_cast_kernel,
// surface_occlusion_kernel): a wave owns tiles of 32 points, lane (j, h) = (lane & 31, lane >> 5) holds point j, the two halves gather
// channels [16 h, 16 h + 16).  The gather and the density net are render_device.h's, fed `coord_scale * p` as sample_points_kernel
// feeds them, so every density equals p3d_sample_points' sigma at the same point bit for bit.
#pragma once
#include "render_device.h"

namespace p3d {

// The packed decoder stream into the front of LDS.  The caller places the __syncthreads() (it may stage more before it).
__device__ __forceinline__ void stage_decoder(float* lds, const float* decoder)
{
    for (int i = threadIdx.x; i < kDecoderFloats / 4; i += blockDim.x) ((f32x4*)lds)[i] = ((const f32x4*)decoder)[i];
}

__device__ __forceinline__ rsrc_t plane_rsrc(const RenderArgs& a)
{
    return __builtin_amdgcn_make_buffer_rsrc((void*)a.planes, 0, a.planes_total_bytes, 0x00020000);
}

// Point j of tile t.  raster = R > 0 (R % 8 == 0, tiles_x = R / 4): the points are an R x R image and a tile is an 8 x 4 pixel block
// (8 rows, 4 columns), so the rays of a wave end together and their taps share lines; else 32 consecutive points.
__device__ __forceinline__ unsigned tile_point(unsigned t, int j, int raster, unsigned tiles_x)
{
    if (raster > 0) {
        const unsigned ty = t / tiles_x, tx = t - ty * tiles_x;
        return (ty * 8u + (unsigned)(j & 7)) * (unsigned)raster + tx * 4u + (unsigned)(j >> 3);
    }
    return t * 32u + (unsigned)j;
}

// The density at (x, y, z): layer 1 and the sigma row of net SN.  Every lane of the wave must get here (MFMAs, a cross-half sum).
template <int SN>
__device__ __forceinline__ float sigma_at(const RenderArgs& a, rsrc_t rsrc, unsigned img_off, const float* lds, int lane, int h, float x, float y, float z)
{
    const float cs = a.coord_scale;
    float feat[16];
    gather_features<true>(a, rsrc, img_off, h, cs * x, cs * y, cs * z, feat);
    f32x16 h0, h1;
    mlp_layer1(lds, SN, lane, h, feat, h0, h1);
    return mlp_sigma(lds, h, h0, h1);
}

} // namespace p3d
