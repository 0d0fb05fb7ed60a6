// Triangle setup, coverage and the per-pixel terms of a shade, shared by the mesh renderer (mesh_raster.hip) and the textured shade
// (mesh_atlas.hip).  Conventions (fixed point, swap rule, fill rule, barycentrics, headlight): include/p3d_hip.h, "mesh rendering".
#pragma once
#include "p3d_common.h"

namespace p3d {

constexpr int kCamFloats = P3D_MESH_CAMERA_FLOATS;
static_assert(kCamFloats == 24, "camera row");

struct Tri {
    int idx[3];                                                           // vertex ids, in the order the weights use
    int64_t x[3], y[3];
    float z[3];
    int c0, c1, r0, r1;                                                   // pixel-centre bounding box, clamped to the image
};

// The triangle's setup, shared by every pass: false when it is not drawn (bad index, dropped vertex, zero area, no pixel centre in
// its clamped bounding box).  Vertices 1 and 2 are swapped when E_01(v2) < 0.
__device__ __forceinline__ bool tri_setup(const int4* __restrict__ proj, const int32_t* __restrict__ faces, int64_t t, int nv, int W, int H,
                                          Tri& T)
{
    int* idx = T.idx;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        idx[k] = faces[t * 3 + k];
        if ((unsigned)idx[k] >= (unsigned)nv) return false;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int4 p = proj[idx[k]];
        if (p.w) return false;
        T.x[k] = p.x; T.y[k] = p.y; T.z[k] = __int_as_float(p.z);
    }
    const int64_t area = (T.x[1] - T.x[0]) * (T.y[2] - T.y[0]) - (T.y[1] - T.y[0]) * (T.x[2] - T.x[0]);
    if (area == 0) return false;
    if (area < 0) {
        int64_t s = T.x[1]; T.x[1] = T.x[2]; T.x[2] = s;
        s = T.y[1]; T.y[1] = T.y[2]; T.y[2] = s;
        const float zs = T.z[1]; T.z[1] = T.z[2]; T.z[2] = zs;
        const int is = idx[1]; idx[1] = idx[2]; idx[2] = is;
    }
    const int64_t xmin = min(T.x[0], min(T.x[1], T.x[2])), xmax = max(T.x[0], max(T.x[1], T.x[2]));
    const int64_t ymin = min(T.y[0], min(T.y[1], T.y[2])), ymax = max(T.y[0], max(T.y[1], T.y[2]));
    // centres (c << 8) + 128 inside [min, max]: c from ceil((min - 128) / 256) to floor((max - 128) / 256) (arithmetic shifts floor)
    T.c0 = (int)max<int64_t>((xmin - 128 + 255) >> 8, 0);
    T.c1 = (int)min<int64_t>((xmax - 128) >> 8, W - 1);
    T.r0 = (int)max<int64_t>((ymin - 128 + 255) >> 8, 0);
    T.r1 = (int)min<int64_t>((ymax - 128) >> 8, H - 1);
    return T.c0 <= T.c1 && T.r0 <= T.r1;
}

__device__ __forceinline__ bool owns(int64_t dx, int64_t dy) { return dy < 0 || (dy == 0 && dx > 0); }

// Edge weights at pixel (r, c); true when the pixel centre is covered (top-left rule).
__device__ __forceinline__ bool tri_weights(const Tri& T, int r, int c, int64_t& w0, int64_t& w1, int64_t& w2)
{
    const int64_t px = ((int64_t)c << 8) + 128, py = ((int64_t)r << 8) + 128;
    const int64_t dx0 = T.x[2] - T.x[1], dy0 = T.y[2] - T.y[1];
    const int64_t dx1 = T.x[0] - T.x[2], dy1 = T.y[0] - T.y[2];
    const int64_t dx2 = T.x[1] - T.x[0], dy2 = T.y[1] - T.y[0];
    w0 = dx0 * (py - T.y[1]) - dy0 * (px - T.x[1]);
    w1 = dx1 * (py - T.y[2]) - dy1 * (px - T.x[2]);
    w2 = dx2 * (py - T.y[0]) - dy2 * (px - T.x[0]);
    return (w0 > 0 || (w0 == 0 && owns(dx0, dy0))) && (w1 > 0 || (w1 == 0 && owns(dx1, dy1))) && (w2 > 0 || (w2 == 0 && owns(dx2, dy2)));
}

// Barycentrics of a pixel from its integer edge weights, in T's corner order: orthographic w_i / s, pinhole (w_i / z_i) / q.
__device__ __forceinline__ void tri_barycentrics(const Tri& T, const int64_t (&w)[3], bool ortho, double (&b)[3])
{
#pragma clang fp contract(off)
    const double a0 = (double)w[0], a1 = (double)w[1], a2 = (double)w[2];
    if (ortho) {
        double s = a0 + a1;
        s = s + a2;
        b[0] = a0 / s; b[1] = a1 / s; b[2] = a2 / s;
    } else {
        const double q0 = a0 / (double)T.z[0], q1 = a1 / (double)T.z[1], q2 = a2 / (double)T.z[2];
        double q = q0 + q1;
        q = q + q2;
        b[0] = q0 / q; b[1] = q1 / q; b[2] = q2 / q;
    }
}

// The headlight factor ambient + (1 - ambient) |n . f| of a face: n its world normal, f the forward axis of the camera row `cam`.
__device__ __forceinline__ double tri_headlight(const float* __restrict__ vertices, const int* idx, const float* __restrict__ cam, float ambient)
{
#pragma clang fp contract(off)
    double e1[3], e2[3];
    for (int k = 0; k < 3; ++k) {
        const double o = (double)vertices[(int64_t)idx[0] * 3 + k];
        e1[k] = (double)vertices[(int64_t)idx[1] * 3 + k] - o;
        e2[k] = (double)vertices[(int64_t)idx[2] * 3 + k] - o;
    }
    const double n0 = e1[1] * e2[2] - e1[2] * e2[1], n1 = e1[2] * e2[0] - e1[0] * e2[2], n2 = e1[0] * e2[1] - e1[1] * e2[0];
    const double f0 = (double)cam[2], f1 = (double)cam[6], f2 = (double)cam[10];
    double nn = n0 * n0; nn = nn + n1 * n1; nn = nn + n2 * n2;
    double ff = f0 * f0; ff = ff + f1 * f1; ff = ff + f2 * f2;
    double dot = n0 * f0; dot = dot + n1 * f1; dot = dot + n2 * f2;
    const double den = sqrt(nn) * sqrt(ff);
    const double cosv = den > 0.0 ? fabs(dot) / den : 0.0;
    const double amb = (double)ambient;
    return amb + (1.0 - amb) * cosv;
}

// A shaded channel as a byte: floor(albedo * shade + 0.5) clamped to [0, 255].
__device__ __forceinline__ uint8_t shaded_byte(double albedo, double shade)
{
#pragma clang fp contract(off)
    const double v = floor(albedo * shade + 0.5);
    return (uint8_t)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));
}

} // namespace p3d
