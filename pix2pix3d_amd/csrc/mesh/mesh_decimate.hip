// Quadric-error decimation for gfx950: the four kernels of a round of edge collapses (p3d_mesh.h;
// pix2pix3d_amd/decimate.py).  The rules are the header's; the torch formulation of decimate.py produces the same bytes.
//
// Every kernel is one thread per item, 256 threads a work-group, plain vector loads and stores, no float atomics, and every list walk is
// bounded by its CSR offsets, which are clamped to the list's length; an index outside [0, V) or [0, T) ends the walk's use of that entry
// (list_range, entry checks), so nothing a caller hands over is followed out of bounds.
//
// p3d_mesh_quadrics      a thread per vertex: the fp64 sum of the face quadrics over the vertex -> face list, in list order (ascending face id).
// p3d_mesh_edge_costs    a thread per edge.  The valence of a marching-cubes mesh is about 6, so the two 1-ring walks of an edge are about a dozen
//                        faces and the lanes of a wave leave their loops within a few iterations of each other: a wave per edge would idle 50 lanes
//                        of 64 on such lists.  The cheap tests come first (fixed ends, uses, the link condition by a merge of the two ascending
//                        neighbour lists); only an edge that passes them pays for the 3 x 3 solve and the flip test.
// p3d_mesh_edge_select   three launches: m1 (a vertex's smallest candidate rank over its edges), m2 (the minimum of m1 over the vertex and its
//                        neighbours), then an edge wins where its rank equals m2 at both ends.  Gathers over the CSR lists, no atomics.
// p3d_mesh_collapse      two launches: a thread per edge moves the lower end of an applied edge, merges the quadrics and points the upper end at
//                        the lower one (applied edges share no vertex, so the in-place update is race free); then a thread per face remaps
//                        its corners through `parent` and flags the faces with two equal corners.
#include "../p3d_common.h"
#include "p3d_mesh.h"
#include <math.h>

namespace {

using namespace p3d;

constexpr int kBlock = 256;
constexpr int kQ = P3D_MESH_QUADRIC_DOUBLES;
static_assert(kQ == 10, "a symmetric 4 x 4 matrix");
constexpr int32_t kNoRank = P3D_MESH_NO_RANK;

struct D3 { double x, y, z; };

__device__ __forceinline__ D3 load3(const float* __restrict__ v, int64_t i)
{
    return D3{(double)v[i * 3], (double)v[i * 3 + 1], (double)v[i * 3 + 2]};
}

__device__ __forceinline__ D3 sub3(const D3& u, const D3& v)
{
#pragma clang fp contract(off)
    return D3{u.x - v.x, u.y - v.y, u.z - v.z};
}

__device__ __forceinline__ double dot3(const D3& u, const D3& v)
{
#pragma clang fp contract(off)
    double s = u.x * v.x;
    s = s + u.y * v.y;
    s = s + u.z * v.z;
    return s;
}

__device__ __forceinline__ D3 cross3(const D3& u, const D3& v)
{
#pragma clang fp contract(off)
    const double a = u.y * v.z, b = u.z * v.y, c = u.z * v.x, d = u.x * v.z, e = u.x * v.y, f = u.y * v.x;
    return D3{a - b, c - d, e - f};
}

__device__ __forceinline__ D3 normal3(const D3& a, const D3& b, const D3& c) { return cross3(sub3(b, a), sub3(c, a)); }

// The list of v, clamped to [0, n_entries).
__device__ __forceinline__ void list_range(const int64_t* __restrict__ offsets, int64_t v, int64_t n_entries, int64_t& s, int64_t& e)
{
    s = offsets[v];
    e = offsets[v + 1];
    s = s < 0 ? 0 : (s > n_entries ? n_entries : s);
    e = e < s ? s : (e > n_entries ? n_entries : e);
}

// The corners of face f; false when f or a corner is out of range.
__device__ __forceinline__ bool load_face(const int32_t* __restrict__ faces, int32_t f, int nf, int nv, int (&x)[3])
{
    if ((unsigned)f >= (unsigned)nf) return false;
    x[0] = faces[(int64_t)f * 3]; x[1] = faces[(int64_t)f * 3 + 1]; x[2] = faces[(int64_t)f * 3 + 2];
    return (unsigned)x[0] < (unsigned)nv && (unsigned)x[1] < (unsigned)nv && (unsigned)x[2] < (unsigned)nv;
}

// ---- quadrics ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) mesh_quadrics_kernel(const float* __restrict__ vertices, int nv, const int32_t* __restrict__ faces, int nf,
                                                               const int64_t* __restrict__ vf_offsets, const int32_t* __restrict__ vf_faces,
                                                               double* __restrict__ quadrics)
{
#pragma clang fp contract(off)
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    double q[kQ];
#pragma unroll
    for (int k = 0; k < kQ; ++k) q[k] = 0.0;
    int64_t s, e;
    list_range(vf_offsets, v, (int64_t)nf * 3, s, e);
    for (int64_t i = s; i < e; ++i) {                                       // list order: ascending face id
        int x[3];
        if (!load_face(faces, vf_faces[i], nf, nv, x)) continue;
        const D3 a = load3(vertices, x[0]), b = load3(vertices, x[1]), c = load3(vertices, x[2]);
        const D3 n = normal3(a, b, c);
        const double nn = dot3(n, n);
        if (!(nn > 0.0)) continue;                                          // a face without area adds nothing
        const double len = sqrt(nn);
        const D3 h = D3{n.x / len, n.y / len, n.z / len};
        const double d = -dot3(h, a);
        const double w = len * 0.5;
        const double p[4] = {h.x, h.y, h.z, d};
        int k = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c2 = r; c2 < 4; ++c2) {
                const double t = p[r] * p[c2];
                q[k] = q[k] + w * t;
                ++k;
            }
    }
#pragma unroll
    for (int k = 0; k < kQ; ++k) quadrics[v * kQ + k] = q[k];
}

// ---- edge costs ----------------------------------------------------------------------------------------------------------------------
// p^T Q p for p = (x, y, z, 1), clamped at 0, in the header's order.
__device__ __forceinline__ double quadric_cost(const double (&q)[kQ], const D3& p)
{
#pragma clang fp contract(off)
    double r0 = q[0] * p.x; r0 = r0 + q[1] * p.y; r0 = r0 + q[2] * p.z; r0 = r0 + q[3];
    double r1 = q[1] * p.x; r1 = r1 + q[4] * p.y; r1 = r1 + q[5] * p.z; r1 = r1 + q[6];
    double r2 = q[2] * p.x; r2 = r2 + q[5] * p.y; r2 = r2 + q[7] * p.z; r2 = r2 + q[8];
    double r3 = q[3] * p.x; r3 = r3 + q[6] * p.y; r3 = r3 + q[8] * p.z; r3 = r3 + q[9];
    double c = p.x * r0; c = c + p.y * r1; c = c + p.z * r2; c = c + r3;
    return c > 0.0 ? c : 0.0;
}

struct EdgeArgs {
    const float* vertices; const double* quadrics; int nv;
    const int32_t* faces; int nf;
    const int64_t* adj_offsets; const int32_t* neighbours; int64_t n_entries;
    const uint8_t* fixed;
    const int64_t* vf_offsets; const int32_t* vf_faces;
    const int32_t* edges; int ne;
    float* target; double* cost; uint8_t* valid;
};

// The flip test over the faces of v that do not use `other`, v moving to p.
__device__ __forceinline__ bool ring_keeps_its_side(const EdgeArgs& g, int v, int other, const D3& p)
{
#pragma clang fp contract(off)
    int64_t s, e;
    list_range(g.vf_offsets, v, (int64_t)g.nf * 3, s, e);
    bool ok = true;
    for (int64_t i = s; i < e; ++i) {
        int x[3];
        if (!load_face(g.faces, g.vf_faces[i], g.nf, g.nv, x)) continue;
        if (x[0] == other || x[1] == other || x[2] == other) continue;
        const D3 a = load3(g.vertices, x[0]), b = load3(g.vertices, x[1]), c = load3(g.vertices, x[2]);
        const D3 n0 = normal3(a, b, c);
        const double nn0 = dot3(n0, n0);
        if (!(nn0 > 0.0)) continue;
        const D3 n1 = normal3(x[0] == v ? p : a, x[1] == v ? p : b, x[2] == v ? p : c);
        const double nn1 = dot3(n1, n1), d = dot3(n0, n1);
        const double lhs = d * d, rhs = (nn0 * nn1) * 0.0625;
        ok = ok && d > 0.0 && lhs >= rhs;
    }
    return ok;
}

__global__ void __launch_bounds__(kBlock) mesh_edge_costs_kernel(const EdgeArgs g)
{
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= g.ne) return;
    const int a = g.edges[e * 2], b = g.edges[e * 2 + 1];
    bool ok = (unsigned)a < (unsigned)g.nv && (unsigned)b < (unsigned)g.nv && a != b;
    if (ok) ok = g.fixed[a] == 0 && g.fixed[b] == 0;
    int t0 = -1, t1 = -1;
    if (ok) {                                                              // the faces that use the edge, and their third corners
        int uses = 0;
        int64_t s, t;
        list_range(g.vf_offsets, a, (int64_t)g.nf * 3, s, t);
        for (int64_t i = s; i < t; ++i) {
            int x[3];
            if (!load_face(g.faces, g.vf_faces[i], g.nf, g.nv, x)) continue;
            if (x[0] != b && x[1] != b && x[2] != b) continue;
            const bool e0 = x[0] == a || x[0] == b, e1 = x[1] == a || x[1] == b;
            const int third = !e0 ? x[0] : (!e1 ? x[1] : x[2]);      // the first corner that is neither end
            if (uses == 0) t0 = third; else if (uses == 1) t1 = third;
            ++uses;
        }
        ok = uses == 2 && t0 != t1;
    }
    if (ok) {                                                              // the link condition: a merge of the two ascending lists
        int64_t i, ie, j, je;
        list_range(g.adj_offsets, a, g.n_entries, i, ie);
        list_range(g.adj_offsets, b, g.n_entries, j, je);
        int common = 0, lo = -1, hi = -1;
        int64_t min_degree = INT64_MAX;
        const int64_t merged_degree = (ie - i) + (je - j) - 4;             // of the merged vertex, once the two common neighbours are known
        while (i < ie && j < je) {
            const int u = g.neighbours[i], w = g.neighbours[j];
            if (u == w) {
                if (common == 0) lo = u;
                hi = u;
                ++common;
                if ((unsigned)u < (unsigned)g.nv) {
                    int64_t cs, ce;
                    list_range(g.adj_offsets, u, g.n_entries, cs, ce);
                    min_degree = min(min_degree, ce - cs);
                } else {
                    min_degree = 0;
                }
                ++i; ++j;
            } else if (u < w) {
                ++i;
            } else {
                ++j;
            }
        }
        ok = common == 2 && lo == min(t0, t1) && hi == max(t0, t1) && min_degree >= 4 && merged_degree >= 4;
    }
    D3 best = D3{0.0, 0.0, 0.0};
    double best_cost = 0.0;
    if (ok) {                                                              // the target point and its cost
        double q[kQ];
#pragma unroll
        for (int k = 0; k < kQ; ++k) q[k] = g.quadrics[(int64_t)a * kQ + k] + g.quadrics[(int64_t)b * kQ + k];
        const D3 pa = load3(g.vertices, a), pb = load3(g.vertices, b);
        const D3 mid = D3{(pa.x + pb.x) * 0.5, (pa.y + pb.y) * 0.5, (pa.z + pb.z) * 0.5};
        best = pa;
        best_cost = quadric_cost(q, pa);
        double c = quadric_cost(q, pb);
        if (c < best_cost) { best = pb; best_cost = c; }
        c = quadric_cost(q, mid);
        if (c < best_cost) { best = mid; best_cost = c; }
        // the minimiser: A x = -(q3, q6, q8), A = [[q0 q1 q2] [q1 q4 q5] [q2 q5 q7]], by cofactors
        const double c00 = q[4] * q[7] - q[5] * q[5], c01 = q[2] * q[5] - q[1] * q[7], c02 = q[1] * q[5] - q[2] * q[4];
        const double c11 = q[0] * q[7] - q[2] * q[2], c12 = q[1] * q[2] - q[0] * q[5], c22 = q[0] * q[4] - q[1] * q[1];
        double det = q[0] * c00; det = det + q[1] * c01; det = det + q[2] * c02;
        double m = fmax(fmax(fmax(fabs(q[0]), fabs(q[1])), fmax(fabs(q[2]), fabs(q[4]))), fmax(fabs(q[5]), fabs(q[7])));
        double bound = m * m; bound = bound * m; bound = bound * 9.5367431640625e-07;      // 2^-20
        if (fabs(det) > bound) {
            double r0 = c00 * q[3]; r0 = r0 + c01 * q[6]; r0 = r0 + c02 * q[8];
            double r1 = c01 * q[3]; r1 = r1 + c11 * q[6]; r1 = r1 + c12 * q[8];
            double r2 = c02 * q[3]; r2 = r2 + c12 * q[6]; r2 = r2 + c22 * q[8];
            const D3 x = D3{(-r0) / det, (-r1) / det, (-r2) / det};
            const D3 off = sub3(x, mid), ab = sub3(pb, pa);
            const double away = dot3(off, off), reach = dot3(ab, ab) * 4.0;
            if (away <= reach) {
                c = quadric_cost(q, x);
                if (c < best_cost) { best = x; best_cost = c; }
            }
        }
        ok = best_cost < INFINITY;
    }
    float tx = 0.f, ty = 0.f, tz = 0.f;
    if (ok) {                                                              // the flip test at the position the vertex would get: fp32
        tx = (float)best.x; ty = (float)best.y; tz = (float)best.z;
        const D3 p = D3{(double)tx, (double)ty, (double)tz};
        ok = ring_keeps_its_side(g, a, b, p) && ring_keeps_its_side(g, b, a, p);
    }
    g.target[e * 3] = ok ? tx : 0.f;
    g.target[e * 3 + 1] = ok ? ty : 0.f;
    g.target[e * 3 + 2] = ok ? tz : 0.f;
    g.cost[e] = ok ? best_cost : (double)INFINITY;
    g.valid[e] = ok ? 1 : 0;
}

// ---- independent set -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) mesh_select_m1_kernel(const int32_t* __restrict__ rank, int ne, int nv, const int64_t* __restrict__ offsets,
                                                                const int32_t* __restrict__ entry_edge, int64_t n_entries, int32_t* __restrict__ m1)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    int64_t s, e;
    list_range(offsets, v, n_entries, s, e);
    int32_t best = kNoRank;
    for (int64_t i = s; i < e; ++i) {
        const int32_t edge = entry_edge[i];
        if ((unsigned)edge < (unsigned)ne) best = min(best, rank[edge]);
    }
    m1[v] = best;
}

__global__ void __launch_bounds__(kBlock) mesh_select_m2_kernel(const int32_t* __restrict__ m1, int nv, const int64_t* __restrict__ offsets,
                                                                const int32_t* __restrict__ neighbours, int64_t n_entries, int32_t* __restrict__ m2)
{
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    int64_t s, e;
    list_range(offsets, v, n_entries, s, e);
    int32_t best = m1[v];
    for (int64_t i = s; i < e; ++i) {
        const int32_t w = neighbours[i];
        if ((unsigned)w < (unsigned)nv) best = min(best, m1[w]);
    }
    m2[v] = best;
}

__global__ void __launch_bounds__(kBlock) mesh_select_win_kernel(const int32_t* __restrict__ rank, const int32_t* __restrict__ edges, int ne, int nv,
                                                                 const int32_t* __restrict__ m2, uint8_t* __restrict__ win)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= ne) return;
    const int a = edges[e * 2], b = edges[e * 2 + 1];
    const int32_t r = rank[e];
    const bool in = (unsigned)a < (unsigned)nv && (unsigned)b < (unsigned)nv;
    win[e] = (in && r != kNoRank && r == m2[in ? a : 0] && r == m2[in ? b : 0]) ? 1 : 0;
}

// ---- collapse ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) mesh_collapse_edges_kernel(float* __restrict__ vertices, double* __restrict__ quadrics,
                                                                     int32_t* __restrict__ parent, int nv, const int32_t* __restrict__ edges,
                                                                     const uint8_t* __restrict__ apply, const float* __restrict__ target, int ne)
{
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= ne || apply[e] == 0) return;
    const int a = edges[e * 2], b = edges[e * 2 + 1];
    if ((unsigned)a >= (unsigned)nv || (unsigned)b >= (unsigned)nv || a == b) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) vertices[(int64_t)a * 3 + k] = target[e * 3 + k];
#pragma unroll
    for (int k = 0; k < kQ; ++k) quadrics[(int64_t)a * kQ + k] = quadrics[(int64_t)a * kQ + k] + quadrics[(int64_t)b * kQ + k];
    parent[b] = a;
}

__global__ void __launch_bounds__(kBlock) mesh_collapse_faces_kernel(const int32_t* __restrict__ parent, int nv, int32_t* __restrict__ faces, int nf,
                                                                     uint8_t* __restrict__ dead)
{
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= nf) return;
    int x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x[k] = faces[f * 3 + k];
        if ((unsigned)x[k] < (unsigned)nv) x[k] = parent[x[k]];
        faces[f * 3 + k] = x[k];
    }
    dead[f] = (x[0] == x[1] || x[1] == x[2] || x[0] == x[2]) ? 1 : 0;
}

bool counts_ok(int64_t n) { return n >= 0 && n < P3D_MESH_DECIMATE_MAX; }
unsigned blocks_for(int64_t n) { return (unsigned)ceil_div(n, kBlock); }

} // namespace

extern "C" int p3d_mesh_quadrics(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces, const int64_t* vf_offsets,
                                 const int32_t* vf_faces, double* quadrics, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(counts_ok(n_vertices) && counts_ok(n_faces), "mesh_quadrics: n_vertices and n_faces are 0 .. %d (got %d, %d)", P3D_MESH_DECIMATE_MAX - 1,
                n_vertices, n_faces);
    if (n_vertices == 0) return P3D_OK;
    P3D_REQUIRE(vertices && vf_offsets && quadrics && (n_faces == 0 || (faces && vf_faces)), "mesh_quadrics: a pointer is null");
    P3D_REQUIRE(((uintptr_t)quadrics & 7u) == 0 && ((uintptr_t)vf_offsets & 7u) == 0, "mesh_quadrics: quadrics and vf_offsets must be 8-byte aligned");
    hipLaunchKernelGGL(mesh_quadrics_kernel, dim3(blocks_for(n_vertices)), dim3(kBlock), 0, (hipStream_t)stream, vertices, n_vertices, faces, n_faces,
                       vf_offsets, vf_faces, quadrics);
    count_launch(FAM_AUX);
    return check_launch("mesh_quadrics");
}

extern "C" int p3d_mesh_edge_costs(const float* vertices, const double* quadrics, int32_t n_vertices, const int32_t* faces, int32_t n_faces,
                                   const int64_t* adj_offsets, const int32_t* neighbours, int64_t n_entries, const uint8_t* fixed,
                                   const int64_t* vf_offsets, const int32_t* vf_faces, const int32_t* edges, int32_t n_edges, float* target,
                                   double* cost, uint8_t* valid, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(counts_ok(n_vertices) && counts_ok(n_faces) && counts_ok(n_edges) && n_entries >= 0,
                "mesh_edge_costs: the counts are 0 .. %d (got %d vertices, %d faces, %d edges, %lld entries)", P3D_MESH_DECIMATE_MAX - 1, n_vertices, n_faces,
                n_edges, (long long)n_entries);
    if (n_edges == 0) return P3D_OK;
    P3D_REQUIRE(vertices && quadrics && faces && adj_offsets && neighbours && fixed && vf_offsets && vf_faces && edges && target && cost && valid,
                "mesh_edge_costs: a pointer is null");
    P3D_REQUIRE(n_vertices > 0 && n_faces > 0, "mesh_edge_costs: edges without vertices or faces");
    P3D_REQUIRE(((uintptr_t)quadrics & 7u) == 0 && ((uintptr_t)cost & 7u) == 0 && ((uintptr_t)adj_offsets & 7u) == 0 && ((uintptr_t)vf_offsets & 7u) == 0,
                "mesh_edge_costs: quadrics, cost and the offsets must be 8-byte aligned");
    EdgeArgs g;
    g.vertices = vertices; g.quadrics = quadrics; g.nv = n_vertices; g.faces = faces; g.nf = n_faces;
    g.adj_offsets = adj_offsets; g.neighbours = neighbours; g.n_entries = n_entries; g.fixed = fixed;
    g.vf_offsets = vf_offsets; g.vf_faces = vf_faces; g.edges = edges; g.ne = n_edges; g.target = target; g.cost = cost; g.valid = valid;
    hipLaunchKernelGGL(mesh_edge_costs_kernel, dim3(blocks_for(n_edges)), dim3(kBlock), 0, (hipStream_t)stream, g);
    count_launch(FAM_AUX);
    return check_launch("mesh_edge_costs");
}

extern "C" int p3d_mesh_edge_select(const int32_t* rank, const int32_t* edges, int32_t n_edges, int32_t n_vertices, const int64_t* adj_offsets,
                                    const int32_t* neighbours, const int32_t* entry_edge, int64_t n_entries, int32_t* m1, int32_t* m2, uint8_t* win,
                                    p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(counts_ok(n_vertices) && counts_ok(n_edges) && n_entries >= 0, "mesh_edge_select: the counts are 0 .. %d (got %d vertices, %d edges, %lld entries)",
                P3D_MESH_DECIMATE_MAX - 1, n_vertices, n_edges, (long long)n_entries);
    if (n_edges == 0 || n_vertices == 0) return P3D_OK;
    P3D_REQUIRE(rank && edges && adj_offsets && neighbours && entry_edge && m1 && m2 && win, "mesh_edge_select: a pointer is null");
    P3D_REQUIRE(((uintptr_t)adj_offsets & 7u) == 0, "mesh_edge_select: adj_offsets must be 8-byte aligned");
    P3D_REQUIRE(m1 != m2, "mesh_edge_select: m1 and m2 are two buffers");
    hipLaunchKernelGGL(mesh_select_m1_kernel, dim3(blocks_for(n_vertices)), dim3(kBlock), 0, (hipStream_t)stream, rank, n_edges, n_vertices, adj_offsets,
                       entry_edge, n_entries, m1);
    count_launch(FAM_AUX);
    hipLaunchKernelGGL(mesh_select_m2_kernel, dim3(blocks_for(n_vertices)), dim3(kBlock), 0, (hipStream_t)stream, m1, n_vertices, adj_offsets, neighbours,
                       n_entries, m2);
    count_launch(FAM_AUX);
    hipLaunchKernelGGL(mesh_select_win_kernel, dim3(blocks_for(n_edges)), dim3(kBlock), 0, (hipStream_t)stream, rank, edges, n_edges, n_vertices, m2, win);
    count_launch(FAM_AUX);
    return check_launch("mesh_edge_select");
}

extern "C" int p3d_mesh_collapse(float* vertices, double* quadrics, int32_t* parent, int32_t n_vertices, int32_t* faces, int32_t n_faces,
                                 const int32_t* edges, const uint8_t* apply, const float* target, int32_t n_edges, uint8_t* dead, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(counts_ok(n_vertices) && counts_ok(n_faces) && counts_ok(n_edges), "mesh_collapse: the counts are 0 .. %d (got %d vertices, %d faces, %d edges)",
                P3D_MESH_DECIMATE_MAX - 1, n_vertices, n_faces, n_edges);
    if (n_faces == 0 || n_vertices == 0) return P3D_OK;
    P3D_REQUIRE(vertices && quadrics && parent && faces && dead && (n_edges == 0 || (edges && apply && target)), "mesh_collapse: a pointer is null");
    P3D_REQUIRE(((uintptr_t)quadrics & 7u) == 0, "mesh_collapse: quadrics must be 8-byte aligned");
    if (n_edges > 0) {
        hipLaunchKernelGGL(mesh_collapse_edges_kernel, dim3(blocks_for(n_edges)), dim3(kBlock), 0, (hipStream_t)stream, vertices, quadrics, parent, n_vertices,
                           edges, apply, target, n_edges);
        count_launch(FAM_AUX);
    }
    hipLaunchKernelGGL(mesh_collapse_faces_kernel, dim3(blocks_for(n_faces)), dim3(kBlock), 0, (hipStream_t)stream, parent, n_vertices, faces, n_faces, dead);
    count_launch(FAM_AUX);
    return check_launch("mesh_collapse");
}
