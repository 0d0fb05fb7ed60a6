// Per-vertex colours from rendered views for gfx950: area-weighted vertex normals and the projection of F frames onto the vertices
// of a mesh (include/p3d_hip.h, "mesh baking"; pix2pix3d_amd/texture.py).  One thread per vertex in every kernel; every sum runs in
// fp64 in a fixed order (corners by ascending face id, views by ascending frame), so the output is a pure function of the inputs and
// equals the operation-by-operation CPU formulation of texture.py byte for byte.
//
// p3d_mesh_vertex_normals: a vertex walks its corner list (a CSR the caller builds with a stable sort) and sums its faces' cross
// products.  Three dependent gathers per corner (face id -> corner indices -> positions); the next corner's face id and indices are
// fetched under the current corner's arithmetic.
// p3d_mesh_bake_accumulate: a vertex walks the views in order.  Per view one coalesced 16-byte record, then twelve gathers (4 face
// ids, 4 depths, 4 texels) at the record's screen position.  Nothing is loaded under a per-lane branch: every address is clamped into
// its buffer and whether the sample counts is decided afterwards, so the loads of a whole group of kBakeGroup views are issued before
// the first of them is used, and the next group's records travel under the current group's arithmetic.  The two texels of a footprint
// row are 6 contiguous bytes of the [F][H][W][3] frames at any byte offset: they are fetched as 4 + 2 bytes (no byte past the pair is
// touched, so the last pixel pair of the buffer needs no special case).
// p3d_mesh_bake_finish: the weighted mean, rounded to uint8, or the fallback colour.
#include "p3d_common.h"
#include <math.h>

namespace p3d {

constexpr int kBakeBlock = 256;
constexpr int kBakeGroup = 2;                                         // views whose gathers are in flight together (24 gathers + 2 records)
constexpr int kBakeMaxDim = 2048;
constexpr int kBakeCamFloats = P3D_MESH_CAMERA_FLOATS;
static_assert(kBakeCamFloats == 24, "camera row");

// The IEEE (correctly rounded) fp64 square root, which the CPU formulation's sqrt is.  The compiler expands an fp64 sqrt on this target
// into a reciprocal-square-root estimate refined with fmas, which is not promised to round correctly, so its result s is checked
// against the exact residual r = fma(-s, s, x) = x - s * s: the true root lies above the midpoint of s and its successor exactly
// when r > s * (next(s) - s), and at or below the midpoint of s and its predecessor exactly when r <= -s * (s - pred(s)) (r and both
// products are multiples of ulp(s)^2, so the u^2 / 4 of the squared midpoints cannot change either comparison; a root never sits on a
// midpoint).  Two rounds cover an estimate two ulps off.  Arguments outside [2^-500, 2^500] are rescaled by an even power of two
// first, so that no product underflows or overflows.  0, negative, infinite and NaN arguments return what sqrt returns.
__device__ __forceinline__ double sqrt_rn(double x)
{
#pragma clang fp contract(off)
    if (!(x > 0.0) || !isfinite(x)) return sqrt(x);
    double scale = 1.0;
    if (x < 0x1p-500) { x = x * 0x1p+600; scale = 0x1p-300; }
    else if (x > 0x1p+500) { x = x * 0x1p-600; scale = 0x1p+300; }
    double s = sqrt(x);
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        const double r = fma(-s, s, x);
        const double up = __longlong_as_double(__double_as_longlong(s) + 1), dn = __longlong_as_double(__double_as_longlong(s) - 1);
        s = r > s * (up - s) ? up : (r <= -(s * (s - dn)) ? dn : s);
    }
    return s * scale;
}

// ---- vertex normals ------------------------------------------------------------------------------------------------------------
struct Corner { int32_t a, b, c; bool ok; };

// The face of list entry k (clamped into the list, so the load is unconditional) and its three indices.
__device__ __forceinline__ Corner corner_load(const int32_t* __restrict__ corner_face, const int32_t* __restrict__ faces, int64_t k,
                                              int64_t n_corners, int32_t nf, int32_t nv)
{
    const int64_t kc = k < n_corners ? k : n_corners - 1;
    const int32_t t = corner_face[kc];
    const bool face_ok = (unsigned)t < (unsigned)nf;
    const int64_t tc = face_ok ? t : 0;
    Corner c;
    c.a = faces[tc * 3]; c.b = faces[tc * 3 + 1]; c.c = faces[tc * 3 + 2];
    c.ok = face_ok && (unsigned)c.a < (unsigned)nv && (unsigned)c.b < (unsigned)nv && (unsigned)c.c < (unsigned)nv;
    if (!c.ok) c.a = c.b = c.c = 0;
    return c;
}

__global__ void __launch_bounds__(kBakeBlock) vertex_normals_kernel(const float* __restrict__ vertices, int32_t nv,
                                                                    const int32_t* __restrict__ faces, int32_t nf,
                                                                    const int32_t* __restrict__ corner_face, const int64_t* __restrict__ offsets,
                                                                    float* __restrict__ normals)
{
#pragma clang fp contract(off)
    const int64_t v = (int64_t)blockIdx.x * kBakeBlock + threadIdx.x;
    if (v >= nv) return;
    const int64_t n_corners = (int64_t)nf * 3;
    int64_t s = offsets[v], e = offsets[v + 1];
    s = s < 0 ? 0 : s;
    e = e > n_corners ? n_corners : e;
    double x = 0.0, y = 0.0, z = 0.0;
    if (s < e) {
        Corner next = corner_load(corner_face, faces, s, n_corners, nf, nv);
        for (int64_t k = s; k < e; ++k) {                            // ascending (face id, corner): `corner_face` comes from a stable sort
            const Corner cur = next;
            next = corner_load(corner_face, faces, k + 1, n_corners, nf, nv);
            double p[3][3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                p[0][j] = (double)vertices[(int64_t)cur.a * 3 + j];
                p[1][j] = (double)vertices[(int64_t)cur.b * 3 + j];
                p[2][j] = (double)vertices[(int64_t)cur.c * 3 + j];
            }
            const double e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
            const double e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
            const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
            x = cur.ok ? x + nx : x;
            y = cur.ok ? y + ny : y;
            z = cur.ok ? z + nz : z;
        }
    }
    double nn = x * x;
    nn = nn + y * y;
    nn = nn + z * z;
    const double len = sqrt_rn(nn);
    const bool ok = len > 0.0 && isfinite(len);
    const double d = ok ? len : 1.0;
    normals[v * 3] = ok ? (float)(x / d) : 0.0f;
    normals[v * 3 + 1] = ok ? (float)(y / d) : 0.0f;
    normals[v * 3 + 2] = ok ? (float)(z / d) : 0.0f;
}

// ---- baking --------------------------------------------------------------------------------------------------------------------
struct BakeArgs {
    const int4* proj; const int32_t* face_id; const float* depth; const uint8_t* images;
    const float* vertices; const float* normals; const float* cameras;
    int32_t nv, n_frames, ortho, W, H, power;
    double tolerance, min_cos;
    double* acc; int32_t* seen;
};

// What one view's gathers bring back for one vertex.
struct BakeTaps {
    int32_t id[4];
    float dep[4];
    uint32_t lo[2];                                                  // bytes 0..3 of a footprint row's two texels
    uint16_t hi[2];                                                  // bytes 4..5
};

__device__ __forceinline__ int32_t clampi(int32_t x, int32_t lo, int32_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

// Issue the twelve gathers of view f at the record's footprint, clamped into the frame (W, H >= 2: the entry point sees to it).
__device__ __forceinline__ void bake_gather(const BakeArgs& a, int f, const int4& rec, BakeTaps& t)
{
    const int32_t c0 = clampi((rec.x - 128) >> 8, 0, a.W - 2), r0 = clampi((rec.y - 128) >> 8, 0, a.H - 2);
    const int64_t pix = ((int64_t)f * a.H + r0) * a.W + c0;
    t.id[0] = a.face_id[pix];        t.id[1] = a.face_id[pix + 1];
    t.id[2] = a.face_id[pix + a.W];  t.id[3] = a.face_id[pix + a.W + 1];
    t.dep[0] = a.depth[pix];         t.dep[1] = a.depth[pix + 1];
    t.dep[2] = a.depth[pix + a.W];   t.dep[3] = a.depth[pix + a.W + 1];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint8_t* p = a.images + (pix + (int64_t)r * a.W) * 3;
        __builtin_memcpy(&t.lo[r], p, 4);
        __builtin_memcpy(&t.hi[r], p + 4, 2);
    }
}

__global__ void __launch_bounds__(kBakeBlock) bake_accumulate_kernel(BakeArgs a)
{
#pragma clang fp contract(off)
    const int64_t v = (int64_t)blockIdx.x * kBakeBlock + threadIdx.x;
    if (v >= a.nv) return;
    const double px = (double)a.vertices[v * 3], py = (double)a.vertices[v * 3 + 1], pz = (double)a.vertices[v * 3 + 2];
    const double nx = (double)a.normals[v * 3], ny = (double)a.normals[v * 3 + 1], nz = (double)a.normals[v * 3 + 2];
    double nn = nx * nx;
    nn = nn + ny * ny;
    nn = nn + nz * nz;
    const double nlen = sqrt_rn(nn);
    double ar = a.acc[v * 4], ag = a.acc[v * 4 + 1], ab = a.acc[v * 4 + 2], aw = a.acc[v * 4 + 3];
    int32_t seen = a.seen[v];
    const int last = a.n_frames - 1;

    int4 rec[kBakeGroup], nrec[kBakeGroup];
#pragma unroll
    for (int j = 0; j < kBakeGroup; ++j) rec[j] = a.proj[(int64_t)min(j, last) * a.nv + v];
    for (int f0 = 0; f0 < a.n_frames; f0 += kBakeGroup) {
        BakeTaps taps[kBakeGroup];
#pragma unroll
        for (int j = 0; j < kBakeGroup; ++j) bake_gather(a, min(f0 + j, last), rec[j], taps[j]);
#pragma unroll
        for (int j = 0; j < kBakeGroup; ++j) nrec[j] = a.proj[(int64_t)min(f0 + kBakeGroup + j, last) * a.nv + v];
#pragma unroll
        for (int j = 0; j < kBakeGroup; ++j) {
            const int f = f0 + j;                                    // wave-uniform
            const float* cam = a.cameras + (int64_t)min(f, last) * kBakeCamFloats;
            const int4 r = rec[j];
            const BakeTaps& t = taps[j];
            const int32_t tx = r.x - 128, ty = r.y - 128;
            const int32_t c0 = tx >> 8, r0 = ty >> 8, fx = tx & 255, fy = ty & 255;
            bool counts = f < a.n_frames && r.w == 0 && c0 >= 0 && r0 >= 0 && c0 + 1 <= a.W - 1 && r0 + 1 <= a.H - 1;
            counts = counts && t.id[0] >= 0 && t.id[1] >= 0 && t.id[2] >= 0 && t.id[3] >= 0;
            const float dmin = fminf(fminf(t.dep[0], t.dep[1]), fminf(t.dep[2], t.dep[3]));
            counts = counts && (double)__int_as_float(r.z) <= (double)dmin + a.tolerance;
            double dx, dy, dz;
            if (a.ortho) {
                dx = -(double)cam[2]; dy = -(double)cam[6]; dz = -(double)cam[10];
            } else {
                dx = (double)cam[3] - px; dy = (double)cam[7] - py; dz = (double)cam[11] - pz;
            }
            double dot = nx * dx;
            dot = dot + ny * dy;
            dot = dot + nz * dz;
            double dd = dx * dx;
            dd = dd + dy * dy;
            dd = dd + dz * dz;
            const double den = nlen * sqrt_rn(dd);
            const double cosv = den > 0.0 ? fabs(dot) / den : 0.0;
            counts = counts && cosv >= a.min_cos;
            double w = cosv;
            for (int k = 1; k < a.power; ++k) w = w * cosv;
            const int32_t w00 = (256 - fy) * (256 - fx), w01 = (256 - fy) * fx, w10 = fy * (256 - fx), w11 = fy * fx;
            const uint32_t b0[6] = {t.lo[0] & 255u, (t.lo[0] >> 8) & 255u, (t.lo[0] >> 16) & 255u, t.lo[0] >> 24, t.hi[0] & 255u, (uint32_t)t.hi[0] >> 8};
            const uint32_t b1[6] = {t.lo[1] & 255u, (t.lo[1] >> 8) & 255u, (t.lo[1] >> 16) & 255u, t.lo[1] >> 24, t.hi[1] & 255u, (uint32_t)t.hi[1] >> 8};
            double col[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int32_t num = w00 * (int32_t)b0[ch] + w01 * (int32_t)b0[3 + ch] + w10 * (int32_t)b1[ch] + w11 * (int32_t)b1[3 + ch];
                col[ch] = (double)num / 65536.0;
            }
            ar = counts ? ar + w * col[0] : ar;
            ag = counts ? ag + w * col[1] : ag;
            ab = counts ? ab + w * col[2] : ab;
            aw = counts ? aw + w : aw;
            seen += counts ? 1 : 0;
        }
#pragma unroll
        for (int j = 0; j < kBakeGroup; ++j) rec[j] = nrec[j];
    }
    a.acc[v * 4] = ar; a.acc[v * 4 + 1] = ag; a.acc[v * 4 + 2] = ab; a.acc[v * 4 + 3] = aw;
    a.seen[v] = seen;
}

__global__ void __launch_bounds__(kBakeBlock) bake_finish_kernel(const double* __restrict__ acc, int32_t nv, const uint8_t* __restrict__ fallback,
                                                                 int32_t fb_r, int32_t fb_g, int32_t fb_b, uint8_t* __restrict__ colors)
{
#pragma clang fp contract(off)
    const int64_t v = (int64_t)blockIdx.x * kBakeBlock + threadIdx.x;
    if (v >= nv) return;
    const double w = acc[v * 4 + 3];
    const bool have = w > 0.0;
    const double d = have ? w : 1.0;
    const int32_t fb[3] = {fb_r, fb_g, fb_b};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double q = floor(acc[v * 4 + ch] / d + 0.5);
        const uint8_t mean = (uint8_t)(q >= 0.0 ? (q > 255.0 ? 255.0 : q) : 0.0);      // (NaN -> 0)
        const uint8_t other = fallback ? fallback[v * 3 + ch] : (uint8_t)fb[ch];
        colors[v * 3 + ch] = have ? mean : other;
    }
}

static int bake_vertices(int32_t nv, const char* what)
{
    P3D_REQUIRE(nv >= 0, "%s: negative vertex count %d", what, nv);
    if (nv > INT32_MAX - 1) return fail(P3D_ERR_UNSUPPORTED, "%s: at most INT32_MAX - 1 vertices (got %d)", what, nv);
    return P3D_OK;
}

static inline unsigned bake_blocks(int64_t n) { return (unsigned)((n + kBakeBlock - 1) / kBakeBlock); }

} // namespace p3d

using namespace p3d;

extern "C" int p3d_mesh_vertex_normals(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces,
                                       const int32_t* corner_face, const int64_t* offsets, float* normals, p3d_stream_t stream)
{
    int rc = bake_vertices(n_vertices, "mesh_vertex_normals");
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(n_faces >= 0, "mesh_vertex_normals: negative face count %d", n_faces);
    if (n_faces > INT32_MAX - 1) return fail(P3D_ERR_UNSUPPORTED, "mesh_vertex_normals: at most INT32_MAX - 1 faces (got %d)", n_faces);
    if (n_vertices == 0) return P3D_OK;
    P3D_REQUIRE(vertices && offsets && normals && (n_faces == 0 || (faces && corner_face)), "mesh_vertex_normals: null pointer");
    hipLaunchKernelGGL(vertex_normals_kernel, dim3(bake_blocks(n_vertices)), dim3(kBakeBlock), 0, (hipStream_t)stream, vertices, n_vertices,
                       faces, n_faces, corner_face, offsets, normals);
    count_launch(FAM_AUX);
    return check_launch("mesh_vertex_normals");
}

extern "C" int p3d_mesh_bake_accumulate(const int32_t* proj, const int32_t* face_id, const float* depth, const uint8_t* images,
                                        const float* vertices, const float* normals, const float* cameras, int32_t n_vertices,
                                        int32_t n_frames, int32_t orthographic, int32_t width, int32_t height, double tolerance,
                                        double min_cos, int32_t power, double* acc, int32_t* seen, p3d_stream_t stream)
{
    int rc = bake_vertices(n_vertices, "mesh_bake_accumulate");
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(n_frames >= 0 && n_frames <= 65535, "mesh_bake_accumulate: n_frames must be in [0, 65535] (got %d)", n_frames);
    P3D_REQUIRE(width >= 1 && height >= 1 && width <= kBakeMaxDim && height <= kBakeMaxDim,
                "mesh_bake_accumulate: image size %d x %d outside [1, %d]^2", width, height, kBakeMaxDim);
    P3D_REQUIRE(power >= 1 && power <= 8, "mesh_bake_accumulate: power must be in 1 .. 8 (got %d)", power);
    P3D_REQUIRE(isfinite(tolerance) && tolerance >= 0.0, "mesh_bake_accumulate: tolerance must be finite and >= 0 (got %g)", tolerance);
    P3D_REQUIRE(isfinite(min_cos) && min_cos >= 0.0, "mesh_bake_accumulate: min_cos must be finite and >= 0 (got %g)", min_cos);
    if (n_vertices == 0 || n_frames == 0 || width < 2 || height < 2) return P3D_OK;      // (no 2 x 2 footprint fits a frame one pixel wide)
    P3D_REQUIRE(proj && face_id && depth && images && vertices && normals && cameras && acc && seen, "mesh_bake_accumulate: null pointer");
    const BakeArgs a{(const int4*)proj, face_id, depth, images, vertices, normals, cameras, n_vertices, n_frames, orthographic, width, height,
                     power, tolerance, min_cos, acc, seen};
    hipLaunchKernelGGL(bake_accumulate_kernel, dim3(bake_blocks(n_vertices)), dim3(kBakeBlock), 0, (hipStream_t)stream, a);
    count_launch(FAM_AUX);
    return check_launch("mesh_bake_accumulate");
}

extern "C" int p3d_mesh_bake_finish(const double* acc, int32_t n_vertices, const uint8_t* fallback, int32_t fb_r, int32_t fb_g, int32_t fb_b,
                                    uint8_t* colors, p3d_stream_t stream)
{
    int rc = bake_vertices(n_vertices, "mesh_bake_finish");
    if (rc != P3D_OK) return rc;
    if (n_vertices == 0) return P3D_OK;
    P3D_REQUIRE(acc && colors, "mesh_bake_finish: null pointer");
    hipLaunchKernelGGL(bake_finish_kernel, dim3(bake_blocks(n_vertices)), dim3(kBakeBlock), 0, (hipStream_t)stream, acc, n_vertices, fallback,
                       fb_r & 255, fb_g & 255, fb_b & 255, colors);
    count_launch(FAM_AUX);
    return check_launch("mesh_bake_finish");
}
