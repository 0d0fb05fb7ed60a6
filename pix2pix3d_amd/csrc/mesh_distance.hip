// Mesh-to-mesh distances for gfx950: surface samples, a bounding-volume hierarchy over the faces, the closest-triangle query
// (include/p3d_hip.h, "mesh distances", states every rule; pix2pix3d_amd/geometry.py holds the definition the bytes are tested against).
//
// sample_counts / sample_points: one thread per face / per point, plain gathers and stores.
// bvh_keys: one thread per item.  bvh_leaves, bvh_level: one thread per leaf / per node of one level; a level reads only the level
// below it, which an earlier launch wrote.
// closest: one query point per lane, a stack of node ids in LDS laid out [row][lane] (a lane's column lives in its own bank, so a
// push or pop of the whole wave is conflict-free), boxes and corners read as float4.
#include "p3d_common.h"
#include <math.h>

namespace p3d {

constexpr int kDistBlock = 256;
constexpr int kLeaf = P3D_MESH_BVH_LEAF;
constexpr double kKeep = 1.0 - 1.0 / (double)(1 << P3D_MESH_BVH_MARGIN_LOG2);      // box * kKeep > best: pruned

struct D3 { double x, y, z; };

__device__ __forceinline__ D3 d3_load(const float* __restrict__ v, int64_t i) { return D3{(double)v[i * 3], (double)v[i * 3 + 1], (double)v[i * 3 + 2]}; }

__device__ __forceinline__ D3 d3_sub(const D3& u, const D3& v)
{
#pragma clang fp contract(off)
    return D3{u.x - v.x, u.y - v.y, u.z - v.z};
}

__device__ __forceinline__ double d3_dot(const D3& u, const D3& v)
{
#pragma clang fp contract(off)
    double s = u.x * v.x;
    s = s + u.y * v.y;
    s = s + u.z * v.z;
    return s;
}

__device__ __forceinline__ D3 d3_cross(const D3& u, const D3& v)
{
#pragma clang fp contract(off)
    return D3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}

__device__ __forceinline__ double seg_d2(const D3& p, const D3& a, const D3& b)
{
#pragma clang fp contract(off)
    const D3 e = d3_sub(b, a), r = d3_sub(p, a);
    const double den = d3_dot(e, e), num = d3_dot(r, e);
    double t = den > 0.0 ? num / den : 0.0;
    t = fmin(fmax(t, 0.0), 1.0);
    const D3 q{r.x - t * e.x, r.y - t * e.y, r.z - t * e.z};
    return d3_dot(q, q);
}

// The squared distance from p to the box [lo, hi]: the expression of tri_d2's last line and of the query's node test.
__device__ __forceinline__ double box_d2(const D3& p, const D3& lo, const D3& hi)
{
#pragma clang fp contract(off)
    const D3 g{fmax(fmax(lo.x - p.x, p.x - hi.x), 0.0), fmax(fmax(lo.y - p.y, p.y - hi.y), 0.0), fmax(fmax(lo.z - p.z, p.z - hi.z), 0.0)};
    return d3_dot(g, g);
}

__device__ __forceinline__ double tri_d2(const D3& p, const D3& a, const D3& b, const D3& c)
{
#pragma clang fp contract(off)
    const double s = fmin(fmin(seg_d2(p, a, b), seg_d2(p, b, c)), seg_d2(p, c, a));
    const D3 e1 = d3_sub(b, a), e2 = d3_sub(c, a);
    const D3 n = d3_cross(e1, e2);
    const double nn = d3_dot(n, n);
    const D3 ra = d3_sub(p, a), rb = d3_sub(p, b), rc = d3_sub(p, c);
    const double wc = d3_dot(d3_cross(e1, ra), n);
    const double wa = d3_dot(d3_cross(d3_sub(c, b), rb), n);
    const double wb = d3_dot(d3_cross(d3_sub(a, c), rc), n);
    const double h = d3_dot(ra, n);
    const bool inside = nn > 0.0 && wa >= 0.0 && wb >= 0.0 && wc >= 0.0;
    const double plane = inside ? (h * h) / nn : s;
    const double m = fmin(s, plane);
    const D3 lo{fmin(fmin(a.x, b.x), c.x), fmin(fmin(a.y, b.y), c.y), fmin(fmin(a.z, b.z), c.z)};
    const D3 hi{fmax(fmax(a.x, b.x), c.x), fmax(fmax(a.y, b.y), c.y), fmax(fmax(a.z, b.z), c.z)};
    return fmax(m, box_d2(p, lo, hi));
}

// The corners of face t when it is valid (indices in range, nine finite coordinates).
__device__ __forceinline__ bool face_corners(const float* __restrict__ vertices, int32_t nv, const int32_t* __restrict__ faces, int64_t t,
                                             D3& a, D3& b, D3& c)
{
    const int32_t ia = faces[t * 3], ib = faces[t * 3 + 1], ic = faces[t * 3 + 2];
    if ((unsigned)ia >= (unsigned)nv || (unsigned)ib >= (unsigned)nv || (unsigned)ic >= (unsigned)nv) return false;
    a = d3_load(vertices, ia); b = d3_load(vertices, ib); c = d3_load(vertices, ic);
    return isfinite(a.x) && isfinite(a.y) && isfinite(a.z) && isfinite(b.x) && isfinite(b.y) && isfinite(b.z) && isfinite(c.x) &&
           isfinite(c.y) && isfinite(c.z);
}

// ---- surface samples ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool spacing_reaches(int32_t k, double s2, double l2)
{
#pragma clang fp contract(off)
    return (double)((int64_t)k * k) * s2 >= l2;
}

__global__ void __launch_bounds__(kDistBlock) sample_counts_kernel(const float* __restrict__ vertices, int32_t nv, const int32_t* __restrict__ faces,
                                                                   int32_t nf, double s2, int32_t k_max, int32_t* __restrict__ k_out,
                                                                   uint8_t* __restrict__ capped)
{
    const int64_t t = (int64_t)blockIdx.x * kDistBlock + threadIdx.x;
    if (t >= nf) return;
    D3 a, b, c;
    if (!face_corners(vertices, nv, faces, t, a, b, c)) { k_out[t] = 0; capped[t] = 0; return; }
    const D3 e0 = d3_sub(b, a), e1 = d3_sub(c, b), e2 = d3_sub(a, c);
    const double l2 = fmax(fmax(d3_dot(e0, e0), d3_dot(e1, e1)), d3_dot(e2, e2));
    const bool over = !spacing_reaches(k_max, s2, l2);
    int32_t lo = 1, hi = k_max;                                      // the smallest k in [lo, hi] that reaches, given that hi does (or is the cap)
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (spacing_reaches(mid, s2, l2)) hi = mid; else lo = mid + 1;
    }
    k_out[t] = over ? k_max : lo;
    capped[t] = (uint8_t)over;
}

__global__ void __launch_bounds__(kDistBlock) sample_points_kernel(const float* __restrict__ vertices, int32_t nv, const int32_t* __restrict__ faces,
                                                                   int32_t nf, const int32_t* __restrict__ k_in, const int64_t* __restrict__ offsets,
                                                                   int64_t n_points, float* __restrict__ points, int32_t* __restrict__ face)
{
#pragma clang fp contract(off)
    const int64_t n = (int64_t)blockIdx.x * kDistBlock + threadIdx.x;
    if (n >= n_points) return;
    int64_t lo = 0, hi = nf;                                         // the last f in [0, nf) with offsets[f] <= n
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= n) lo = mid; else hi = mid;
    }
    const int64_t f = lo;
    const int32_t k = min(max(k_in[f], 1), P3D_MESH_SAMPLE_KMAX);
    int64_t r = n - offsets[f];
    D3 a, b, c;
    const bool ok = r >= 0 && r < (int64_t)k * k && face_corners(vertices, nv, faces, f, a, b, c);
    if (!ok) {                                                       // (offsets that are not the scan of k * k: nothing to read, a defined answer)
        points[n * 3] = 0.f; points[n * 3 + 1] = 0.f; points[n * 3 + 2] = 0.f; face[n] = -1;
        return;
    }
    const int64_t upright = (int64_t)k * (k + 1) / 2;
    int32_t add = 1, rows = k;                                       // upright: rows of k, k - 1, ..., 1; inverted: k - 1, ..., 1
    if (r >= upright) { r -= upright; add = 2; rows = k - 1; }
    int32_t i = 0;
    while (i < rows - 1 && r >= rows - i) { r -= rows - i; ++i; }
    const int32_t n0 = 3 * i + add, n1 = 3 * (int32_t)r + add, n2 = 3 * k - n0 - n1;
    const double w0 = (double)n0, w1 = (double)n1, w2 = (double)n2, den = (double)(3 * k);
    double s = w0 * a.x; s = s + w1 * b.x; s = s + w2 * c.x;
    points[n * 3] = (float)(s / den);
    s = w0 * a.y; s = s + w1 * b.y; s = s + w2 * c.y;
    points[n * 3 + 1] = (float)(s / den);
    s = w0 * a.z; s = s + w1 * b.z; s = s + w2 * c.z;
    points[n * 3 + 2] = (float)(s / den);
    face[n] = (int32_t)f;
}

// ---- the hierarchy --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t morton_axis(double c, float lo, float hi)
{
#pragma clang fp contract(off)
    const double ext = 3.0 * ((double)hi - (double)lo);
    if (!(ext > 0.0) || !isfinite(ext)) return 0;
    const double q = floor((c - 3.0 * (double)lo) / ext * 2097152.0);
    return (int64_t)fmin(fmax(q, 0.0), 2097151.0);                   // (a NaN -> 0)
}

__device__ __forceinline__ int64_t morton_spread(int64_t x)          // bit b -> bit 3 b, 21 bits
{
    x &= 0x1fffff;
    x = (x | x << 32) & 0x1f00000000ffffLL;
    x = (x | x << 16) & 0x1f0000ff0000ffLL;
    x = (x | x << 8) & 0x100f00f00f00f00fLL;
    x = (x | x << 4) & 0x10c30c30c30c30c3LL;
    x = (x | x << 2) & 0x1249249249249249LL;
    return x;
}

__global__ void __launch_bounds__(kDistBlock) bvh_keys_kernel(const float* __restrict__ vertices, int32_t nv, const int32_t* __restrict__ faces,
                                                              int32_t n_items, const float* __restrict__ box, int64_t* __restrict__ key)
{
#pragma clang fp contract(off)
    const int64_t t = (int64_t)blockIdx.x * kDistBlock + threadIdx.x;
    if (t >= n_items) return;
    D3 a, b, c;
    bool ok;
    if (faces) ok = face_corners(vertices, nv, faces, t, a, b, c);
    else {
        a = d3_load(vertices, t);
        b = a; c = a;
        ok = isfinite(a.x) && isfinite(a.y) && isfinite(a.z);
    }
    if (!ok) { key[t] = INT64_MAX; return; }
    const int64_t x = morton_axis((a.x + b.x) + c.x, box[0], box[3]);
    const int64_t y = morton_axis((a.y + b.y) + c.y, box[1], box[4]);
    const int64_t z = morton_axis((a.z + b.z) + c.z, box[2], box[5]);
    key[t] = morton_spread(x) | morton_spread(y) << 1 | morton_spread(z) << 2;
}

__global__ void __launch_bounds__(kDistBlock) bvh_leaves_kernel(const float* __restrict__ vertices, int32_t nv, const int32_t* __restrict__ faces,
                                                                int32_t nf, const int32_t* __restrict__ order, int32_t n_leaves, int32_t n_pad,
                                                                float4* __restrict__ tris, float4* __restrict__ nodes)
{
    const int64_t l = (int64_t)blockIdx.x * kDistBlock + threadIdx.x;
    if (l >= n_pad) return;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (l < n_leaves) {
        for (int j = 0; j < kLeaf; ++j) {
            const int64_t slot = l * kLeaf + j;
            int32_t id = -1;
            float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (slot < nf) {
                const int32_t t = order[slot];
                D3 a, b, c;
                if ((unsigned)t < (unsigned)nf && face_corners(vertices, nv, faces, t, a, b, c)) {
                    id = t;
                    v[0] = (float)a.x; v[1] = (float)a.y; v[2] = (float)a.z;      // (exact: they came from fp32)
                    v[3] = (float)b.x; v[4] = (float)b.y; v[5] = (float)b.z;
                    v[6] = (float)c.x; v[7] = (float)c.y; v[8] = (float)c.z;
                    for (int k = 0; k < 3; ++k) {
                        lo[k] = fminf(lo[k], fminf(fminf(v[k], v[3 + k]), v[6 + k]));
                        hi[k] = fmaxf(hi[k], fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k]));
                    }
                }
            }
            tris[slot * 3] = make_float4(v[0], v[1], v[2], __int_as_float(id));
            tris[slot * 3 + 1] = make_float4(v[3], v[4], v[5], 0.f);
            tris[slot * 3 + 2] = make_float4(v[6], v[7], v[8], 0.f);
        }
    }
    const int64_t node = (int64_t)n_pad - 1 + l;
    nodes[node * 2] = make_float4(lo[0], lo[1], lo[2], 0.f);
    nodes[node * 2 + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
}

// Nodes [first, first + count) of one level from their children, which the launch before wrote.
__global__ void __launch_bounds__(kDistBlock) bvh_level_kernel(float4* nodes, int32_t first, int32_t count)
{
    const int64_t j = (int64_t)blockIdx.x * kDistBlock + threadIdx.x;
    if (j >= count) return;
    const int64_t node = (int64_t)first + j, c0 = 2 * node + 1, c1 = c0 + 1;
    const float4 lo0 = nodes[c0 * 2], hi0 = nodes[c0 * 2 + 1], lo1 = nodes[c1 * 2], hi1 = nodes[c1 * 2 + 1];
    nodes[node * 2] = make_float4(fminf(lo0.x, lo1.x), fminf(lo0.y, lo1.y), fminf(lo0.z, lo1.z), 0.f);
    nodes[node * 2 + 1] = make_float4(fmaxf(hi0.x, hi1.x), fmaxf(hi0.y, hi1.y), fmaxf(hi0.z, hi1.z), 0.f);
}

__device__ __forceinline__ double node_d2(const float4* __restrict__ nodes, int32_t node, const D3& p)
{
    const float4 lo = nodes[(int64_t)node * 2], hi = nodes[(int64_t)node * 2 + 1];
    return box_d2(p, D3{(double)lo.x, (double)lo.y, (double)lo.z}, D3{(double)hi.x, (double)hi.y, (double)hi.z});
}

__global__ void __launch_bounds__(kDistBlock) closest_kernel(const float* __restrict__ points, int64_t n_points, const float4* __restrict__ tris,
                                                             const float4* __restrict__ nodes, int32_t n_leaves, int32_t n_pad, int32_t rows,
                                                             double* __restrict__ d2, int64_t* __restrict__ face, int32_t* status)
{
    extern __shared__ int32_t stack[];                               // [rows][kDistBlock]
    const int64_t n = (int64_t)blockIdx.x * kDistBlock + threadIdx.x;
    if (n >= n_points) return;
    const D3 p = d3_load(points, n);
    double best = INFINITY;
    int32_t best_id = -1;
    if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
        const int32_t leaf_base = n_pad - 1;
        const int64_t bound = 2 * (int64_t)n_pad - 1;                // the node count: every node is entered at most once
        int32_t sp = 0, node = 0;
        bool broken = false;
        for (int64_t it = 0; node >= 0; ++it) {
            if (it >= bound) { broken = true; break; }
            if (node >= leaf_base) {
                const int64_t leaf = node - leaf_base;
                if (leaf < n_leaves) {
#pragma unroll
                    for (int j = 0; j < kLeaf; ++j) {
                        const float4 ta = tris[(leaf * kLeaf + j) * 3];
                        const int32_t id = __float_as_int(ta.w);
                        if (id < 0) continue;
                        const float4 tb = tris[(leaf * kLeaf + j) * 3 + 1], tc = tris[(leaf * kLeaf + j) * 3 + 2];
                        const double d = tri_d2(p, D3{(double)ta.x, (double)ta.y, (double)ta.z}, D3{(double)tb.x, (double)tb.y, (double)tb.z},
                                                D3{(double)tc.x, (double)tc.y, (double)tc.z});
                        if (d < best || (d == best && id < best_id)) { best = d; best_id = id; }
                    }
                }
                node = -1;
            } else {
                const int32_t c0 = 2 * node + 1, c1 = c0 + 1;
                const double b0 = node_d2(nodes, c0, p), b1 = node_d2(nodes, c1, p);
                const bool swap = b1 < b0;
                const int32_t nearer = swap ? c1 : c0, farther = swap ? c0 : c1;
                const double bn = swap ? b1 : b0, bf = swap ? b0 : b1;
                if (!(bf * kKeep > best)) {
                    if (sp >= rows) { broken = true; break; }
                    stack[sp * kDistBlock + threadIdx.x] = farther;
                    ++sp;
                }
                node = !(bn * kKeep > best) ? nearer : -1;
            }
            while (node < 0 && sp > 0) {                             // pop until a node that still can hold the minimum
                --sp;
                const int32_t cand = stack[sp * kDistBlock + threadIdx.x];
                if (!(node_d2(nodes, cand, p) * kKeep > best)) node = cand;
            }
        }
        if (broken) { *status = 1; best = INFINITY; best_id = -2; }
    }
    d2[n] = best;
    face[n] = (int64_t)best_id;
}

static int dist_sizes(int32_t n_faces, int32_t n_vertices, const char* what)
{
    P3D_REQUIRE(n_faces >= 0 && n_vertices >= 0, "%s: negative size (%d faces, %d vertices)", what, n_faces, n_vertices);
    if (n_faces > INT32_MAX - 1 || n_vertices > INT32_MAX - 1)
        return fail(P3D_ERR_UNSUPPORTED, "%s: at most INT32_MAX - 1 faces and vertices (got %d, %d)", what, n_faces, n_vertices);
    return P3D_OK;
}

// n_pad must be the power of two the header names for n_faces; depth <- log2(n_pad).
static int dist_tree(int32_t n_faces, int32_t n_pad, const char* what, int* depth)
{
    const int64_t n_leaves = ((int64_t)n_faces + kLeaf - 1) / kLeaf;
    int64_t want = 1;
    int d = 0;
    while (want < n_leaves) { want *= 2; ++d; }
    P3D_REQUIRE(n_pad == want, "%s: n_pad must be %lld for %d faces (got %d)", what, (long long)want, n_faces, n_pad);
    P3D_REQUIRE(d + 1 <= P3D_MESH_BVH_MAX_DEPTH, "%s: tree depth %d beyond %d", what, d + 1, P3D_MESH_BVH_MAX_DEPTH);
    *depth = d;
    return P3D_OK;
}

static inline unsigned dist_blocks(int64_t n) { return (unsigned)((n + kDistBlock - 1) / kDistBlock); }

} // namespace p3d

using namespace p3d;

extern "C" int p3d_mesh_sample_counts(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces, double spacing2,
                                      int32_t k_max, int32_t* k, uint8_t* capped, p3d_stream_t stream)
{
    int rc = dist_sizes(n_faces, n_vertices, "mesh_sample_counts");
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(spacing2 > 0.0 && isfinite(spacing2), "mesh_sample_counts: spacing^2 must be positive and finite (got %g)", spacing2);
    P3D_REQUIRE(k_max >= 1 && k_max <= P3D_MESH_SAMPLE_KMAX, "mesh_sample_counts: k_max must be in [1, %d] (got %d)", P3D_MESH_SAMPLE_KMAX, k_max);
    P3D_REQUIRE(n_faces == 0 || (faces && k && capped && (n_vertices == 0 || vertices)), "mesh_sample_counts: null pointer");
    if (n_faces == 0) return P3D_OK;
    hipLaunchKernelGGL(sample_counts_kernel, dim3(dist_blocks(n_faces)), dim3(kDistBlock), 0, (hipStream_t)stream, vertices, n_vertices, faces,
                       n_faces, spacing2, k_max, k, capped);
    count_launch(FAM_AUX);
    return check_launch("mesh_sample_counts");
}

extern "C" int p3d_mesh_sample_points(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces, const int32_t* k,
                                      const int64_t* offsets, int64_t n_points, float* points, int32_t* face, p3d_stream_t stream)
{
    int rc = dist_sizes(n_faces, n_vertices, "mesh_sample_points");
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(n_points >= 0, "mesh_sample_points: negative point count");
    if (n_points > INT32_MAX - 1) return fail(P3D_ERR_UNSUPPORTED, "mesh_sample_points: at most INT32_MAX - 1 points (got %lld)", (long long)n_points);
    P3D_REQUIRE(n_points == 0 || n_faces > 0, "mesh_sample_points: %lld points of no faces", (long long)n_points);
    P3D_REQUIRE(n_points == 0 || (vertices && faces && k && offsets && points && face), "mesh_sample_points: null pointer");
    if (n_points == 0) return P3D_OK;
    hipLaunchKernelGGL(sample_points_kernel, dim3(dist_blocks(n_points)), dim3(kDistBlock), 0, (hipStream_t)stream, vertices, n_vertices, faces,
                       n_faces, k, offsets, n_points, points, face);
    count_launch(FAM_AUX);
    return check_launch("mesh_sample_points");
}

extern "C" int p3d_mesh_bvh_keys(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_items, const float* box,
                                 int64_t* key, p3d_stream_t stream)
{
    int rc = dist_sizes(n_items, n_vertices, "mesh_bvh_keys");
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(faces || n_items <= n_vertices, "mesh_bvh_keys: %d points of %d vertices", n_items, n_vertices);
    P3D_REQUIRE(n_items == 0 || (box && key && (n_vertices == 0 || vertices)), "mesh_bvh_keys: null pointer");
    if (n_items == 0) return P3D_OK;
    hipLaunchKernelGGL(bvh_keys_kernel, dim3(dist_blocks(n_items)), dim3(kDistBlock), 0, (hipStream_t)stream, vertices, n_vertices, faces, n_items,
                       box, key);
    count_launch(FAM_AUX);
    return check_launch("mesh_bvh_keys");
}

extern "C" int p3d_mesh_bvh_build(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces, const int32_t* order,
                                  int32_t n_pad, float* tris, float* nodes, p3d_stream_t stream)
{
    int rc = dist_sizes(n_faces, n_vertices, "mesh_bvh_build");
    if (rc != P3D_OK) return rc;
    int depth = 0;
    rc = dist_tree(n_faces, n_pad, "mesh_bvh_build", &depth);
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(nodes && (n_faces == 0 || (faces && order && tris && (n_vertices == 0 || vertices))), "mesh_bvh_build: null pointer");
    P3D_REQUIRE(((uintptr_t)nodes & 15u) == 0 && ((uintptr_t)tris & 15u) == 0, "mesh_bvh_build: tris and nodes must be 16-byte aligned");
    const int32_t n_leaves = (int32_t)(((int64_t)n_faces + kLeaf - 1) / kLeaf);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bvh_leaves_kernel, dim3(dist_blocks(n_pad)), dim3(kDistBlock), 0, s, vertices, n_vertices, faces, n_faces, order, n_leaves,
                       n_pad, (float4*)tris, (float4*)nodes);
    count_launch(FAM_AUX);
    rc = check_launch("mesh_bvh_leaves");
    for (int level = depth - 1; level >= 0 && rc == P3D_OK; --level) {
        const int32_t count = (int32_t)1 << level;                   // nodes [2^level - 1, 2^(level + 1) - 1)
        hipLaunchKernelGGL(bvh_level_kernel, dim3(dist_blocks(count)), dim3(kDistBlock), 0, s, (float4*)nodes, count - 1, count);
        count_launch(FAM_AUX);
        rc = check_launch("mesh_bvh_level");
    }
    return rc;
}

extern "C" int p3d_mesh_closest(const float* points, int64_t n_points, const float* tris, const float* nodes, int32_t n_faces, int32_t n_pad,
                                double* d2, int64_t* face, int32_t* status, p3d_stream_t stream)
{
    int rc = dist_sizes(n_faces, 0, "mesh_closest");
    if (rc != P3D_OK) return rc;
    int depth = 0;
    rc = dist_tree(n_faces, n_pad, "mesh_closest", &depth);
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(n_points >= 0, "mesh_closest: negative point count");
    if (n_points > ((int64_t)1 << 38)) return fail(P3D_ERR_UNSUPPORTED, "mesh_closest: at most 2^38 points (got %lld)", (long long)n_points);
    P3D_REQUIRE(n_points == 0 || (points && nodes && d2 && face && status && (n_faces == 0 || tris)), "mesh_closest: null pointer");
    P3D_REQUIRE(((uintptr_t)nodes & 15u) == 0 && ((uintptr_t)tris & 15u) == 0, "mesh_closest: tris and nodes must be 16-byte aligned");
    if (n_points == 0) return P3D_OK;
    const int32_t n_leaves = (int32_t)(((int64_t)n_faces + kLeaf - 1) / kLeaf);
    const int32_t rows = depth + 1;                                  // one farther child per inner level, and one to spare
    hipLaunchKernelGGL(closest_kernel, dim3(dist_blocks(n_points)), dim3(kDistBlock), (size_t)rows * kDistBlock * sizeof(int32_t),
                       (hipStream_t)stream, points, n_points, (const float4*)tris, (const float4*)nodes, n_leaves, n_pad, rows, d2, face, status);
    count_launch(FAM_AUX);
    return check_launch("mesh_closest");
}
