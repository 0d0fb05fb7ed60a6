// Mesh filtering for gfx950: Laplacian / Taubin smoothing of per-vertex attributes, majority voting of per-vertex labels and a shade
// with interpolated vertex normals (include/p3d_hip.h, "mesh filtering"; pix2pix3d_amd/mesh.py).
//
// All three read the mesh through the adjacency lists mesh.adjacency builds with sorts (offsets int64 [V + 1], neighbours int32 [E],
// ascending ids inside a list) or, for the shade, through the raster buffers.  A list is clamped to [0, E) and an entry outside
// [0, V) is skipped, so no index a caller hands over is followed out of bounds.
//
// p3d_mesh_smooth_step: one thread per (vertex, channel), channel fastest: the lanes of a wave that work on one vertex read each
// neighbour's row as one contiguous run.  The fp64 sum of a list runs in list order inside one thread (the loads do not depend on the
// sum and are issued ahead of it), so the bytes are a pure function of the inputs and equal the CPU formulation's.
// p3d_mesh_label_vote: one launch.  A thread whose vertex lists at most P3D_MESH_VOTE_THREAD_DEGREE neighbours counts in its own column
// of an LDS byte table [256 labels][128 threads]: one walk to count, one to find the winner among the labels that occur, one to put
// the zeros back, never a label-by-label or neighbour-by-neighbour comparison.  A vertex with a longer list is put on the work-group's
// list and, after a barrier, counted by the whole group with integer LDS atomics on a 256-entry histogram (order independent).
// p3d_mesh_shade_smooth: p3d_mesh_shade (mesh_raster.hip) with the face normal replaced by the barycentric mix of the vertex normals;
// setup, coverage, barycentrics and rounding are mesh_tri.h's.
#include "mesh_tri.h"
#include <math.h>

namespace p3d {

constexpr int kFilterBlock = 256;
constexpr int kVoteBlock = 128;
constexpr int kVoteLabels = 256;
constexpr int kVoteThreadDegree = P3D_MESH_VOTE_THREAD_DEGREE;
static_assert(kVoteThreadDegree + 1 <= 255, "a byte counts a thread's list and the vertex itself");
static_assert(kVoteBlock >= 4, "the byte table [labels][threads] also holds the group's int32 histogram [labels]");

// The list of v, clamped to [0, n_entries).
__device__ __forceinline__ void list_range(const int64_t* __restrict__ offsets, int64_t v, int64_t n_entries, int64_t& s, int64_t& e)
{
    s = offsets[v];
    e = offsets[v + 1];
    s = s < 0 ? 0 : (s > n_entries ? n_entries : s);
    e = e < s ? s : (e > n_entries ? n_entries : e);
}

__global__ void __launch_bounds__(kFilterBlock) smooth_step_kernel(const float* __restrict__ x, int nv, int C, const int64_t* __restrict__ offsets,
                                                                   const int32_t* __restrict__ neighbours, int64_t n_entries,
                                                                   const uint8_t* __restrict__ pinned, double factor, float* __restrict__ out)
{
#pragma clang fp contract(off)
    const int64_t total = (int64_t)nv * C;
    for (int64_t i = (int64_t)blockIdx.x * kFilterBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kFilterBlock) {
        const int64_t v = i / C;
        const int c = (int)(i - v * C);
        const float own = x[i];
        if (pinned && pinned[v]) { out[i] = own; continue; }
        int64_t s, e;
        list_range(offsets, v, n_entries, s, e);
        double acc = 0.0;
        int64_t degree = 0;
#pragma unroll 4
        for (int64_t k = s; k < e; ++k) {                                 // list order; a skipped entry adds +0.0, which changes nothing
            const int32_t w = neighbours[k];
            const bool ok = (unsigned)w < (unsigned)nv;
            const float xw = x[(int64_t)(ok ? w : 0) * C + c];
            acc = acc + (ok ? (double)xw : 0.0);
            degree += ok ? 1 : 0;
        }
        if (degree == 0) { out[i] = own; continue; }
        const double m = acc / (double)degree;
        const double d = m - (double)own;
        const double p = factor * d;
        const double y = (double)own + p;
        out[i] = (float)y;
    }
}

// The winner of a vote from the counts of the candidate labels: candidates arrive in any order.
struct Vote {
    int count = 0, label = kVoteLabels;
    __device__ __forceinline__ void offer(int c, int l) { if (c > count || (c == count && l < label)) { count = c; label = l; } }
};

__global__ void __launch_bounds__(kVoteBlock) label_vote_kernel(const uint8_t* __restrict__ labels, int nv, const int64_t* __restrict__ offsets,
                                                                const int32_t* __restrict__ neighbours, int64_t n_entries,
                                                                const uint8_t* __restrict__ pinned, uint8_t* __restrict__ out)
{
    __shared__ int32_t words[kVoteLabels * kVoteBlock / 4];               // 32 KiB: bytes [label][thread], then int32 [label]
    __shared__ int32_t big[kVoteBlock];
    __shared__ int n_big;
    const int tid = threadIdx.x;
    for (int i = tid; i < kVoteLabels * kVoteBlock / 4; i += kVoteBlock) words[i] = 0;
    if (tid == 0) n_big = 0;
    __syncthreads();
    uint8_t* col = reinterpret_cast<uint8_t*>(words) + tid;              // count of label l: col[l * kVoteBlock]
    const int64_t v = (int64_t)blockIdx.x * kVoteBlock + tid;
    if (v < nv) {
        const int own = labels[v];
        int64_t s, e;
        list_range(offsets, v, n_entries, s, e);
        if ((pinned && pinned[v]) || e == s) {
            out[v] = (uint8_t)own;
        } else if (e - s > kVoteThreadDegree) {
            big[atomicAdd(&n_big, 1)] = (int32_t)v;
        } else {
            col[own * kVoteBlock] = 1;
            for (int64_t k = s; k < e; ++k) {
                const int32_t w = neighbours[k];
                if ((unsigned)w < (unsigned)nv) col[labels[w] * kVoteBlock] += 1;
            }
            Vote best;
            const int own_count = col[own * kVoteBlock];
            best.offer(own_count, own);
            for (int64_t k = s; k < e; ++k) {
                const int32_t w = neighbours[k];
                if ((unsigned)w >= (unsigned)nv) continue;
                const int l = labels[w];
                best.offer(col[l * kVoteBlock], l);
            }
            out[v] = (uint8_t)(own_count == best.count ? own : best.label);
            col[own * kVoteBlock] = 0;
            for (int64_t k = s; k < e; ++k) {
                const int32_t w = neighbours[k];
                if ((unsigned)w < (unsigned)nv) col[labels[w] * kVoteBlock] = 0;
            }
        }
    }
    __syncthreads();                                                      // the table is all zeros again; n_big is final
    const int n = n_big;
    for (int b = 0; b < n; ++b) {                                        // (uniform: every thread takes every barrier)
        const int64_t u = big[b];
        int64_t s, e;
        list_range(offsets, u, n_entries, s, e);
        for (int64_t k = s + tid; k < e; k += kVoteBlock) {
            const int32_t w = neighbours[k];
            if ((unsigned)w < (unsigned)nv) atomicAdd(&words[labels[w]], 1);
        }
        __syncthreads();
        if (tid == 0) {
            const int own = labels[u];
            const int own_count = words[own] + 1;
            Vote best;
            best.offer(own_count, own);
            for (int l = 0; l < kVoteLabels; ++l) best.offer(l == own ? own_count : words[l], l);
            out[u] = (uint8_t)(own_count == best.count ? own : best.label);
        }
        __syncthreads();
        for (int l = tid; l < kVoteLabels; l += kVoteBlock) words[l] = 0;
        __syncthreads();
    }
}

// The headlight factor of a pixel from interpolated vertex normals: n = b0 n_0 + b1 n_1 + b2 n_2 per component, then tri_headlight's
// dot products, square roots and ambient mix.
__device__ __forceinline__ double smooth_headlight(const float* __restrict__ normals, const int* idx, const double (&b)[3],
                                                   const float* __restrict__ cam, float ambient)
{
#pragma clang fp contract(off)
    double n[3];
    for (int k = 0; k < 3; ++k) {
        double a = b[0] * (double)normals[(int64_t)idx[0] * 3 + k];
        a = a + b[1] * (double)normals[(int64_t)idx[1] * 3 + k];
        a = a + b[2] * (double)normals[(int64_t)idx[2] * 3 + k];
        n[k] = a;
    }
    const double f0 = (double)cam[2], f1 = (double)cam[6], f2 = (double)cam[10];
    double nn = n[0] * n[0]; nn = nn + n[1] * n[1]; nn = nn + n[2] * n[2];
    double ff = f0 * f0; ff = ff + f1 * f1; ff = ff + f2 * f2;
    double dot = n[0] * f0; dot = dot + n[1] * f1; dot = dot + n[2] * f2;
    const double den = sqrt(nn) * sqrt(ff);
    const double cosv = den > 0.0 ? fabs(dot) / den : 0.0;
    const double amb = (double)ambient;
    return amb + (1.0 - amb) * cosv;
}

__global__ void __launch_bounds__(kFilterBlock) mesh_shade_smooth_kernel(const int32_t* __restrict__ face_id, const int4* __restrict__ proj,
                                                                         int nv, const int32_t* __restrict__ faces, int nf,
                                                                         const float* __restrict__ normals, const uint8_t* __restrict__ colors,
                                                                         const float* __restrict__ cameras, int n_frames, int ortho, int W, int H,
                                                                         float ambient, int bg_r, int bg_g, int bg_b, uint8_t* __restrict__ rgb)
{
#pragma clang fp contract(off)
    const int64_t hw = (int64_t)H * W, total = (int64_t)n_frames * hw;
    for (int64_t i = (int64_t)blockIdx.x * kFilterBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kFilterBlock) {
        const int f = (int)(i / hw);
        const int64_t p = i - (int64_t)f * hw;
        const int r = (int)(p / W), c = (int)(p - (int64_t)r * W);
        const int t = face_id[i];
        uint8_t* px = rgb + i * 3;
        Tri T;
        if (t < 0 || t >= nf || !tri_setup(proj + (int64_t)f * nv, faces, t, nv, W, H, T)) {
            px[0] = (uint8_t)bg_r; px[1] = (uint8_t)bg_g; px[2] = (uint8_t)bg_b;
            continue;
        }
        int64_t w[3];
        tri_weights(T, r, c, w[0], w[1], w[2]);
        const int* idx = T.idx;
        double b[3];
        tri_barycentrics(T, w, ortho != 0, b);
        const double shade = smooth_headlight(normals, idx, b, cameras + (int64_t)f * kCamFloats, ambient);
        for (int ch = 0; ch < 3; ++ch) {
            double a;
            if (colors) {
                a = b[0] * (double)colors[(int64_t)idx[0] * 3 + ch];
                a = a + b[1] * (double)colors[(int64_t)idx[1] * 3 + ch];
                a = a + b[2] * (double)colors[(int64_t)idx[2] * 3 + ch];
            } else {
                a = (double)P3D_MESH_GREY;
            }
            px[ch] = shaded_byte(a, shade);
        }
    }
}

static int filter_sizes(int32_t n_vertices, int64_t n_entries, const char* what)
{
    P3D_REQUIRE(n_vertices >= 0 && n_entries >= 0, "%s: negative size (%d vertices, %lld list entries)", what, n_vertices, (long long)n_entries);
    if (n_vertices > INT32_MAX - 1) return fail(P3D_ERR_UNSUPPORTED, "%s: at most INT32_MAX - 1 vertices (got %d)", what, n_vertices);
    return P3D_OK;
}

static bool ranges_overlap(const void* a, const void* b, size_t bytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bytes && b0 < a0 + bytes;
}

static unsigned filter_grid(int64_t work, int64_t cap)
{
    int64_t g = (work + kFilterBlock - 1) / kFilterBlock;
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

} // namespace p3d

using namespace p3d;

extern "C" int p3d_mesh_smooth_step(const float* x, int32_t n_vertices, int32_t channels, const int64_t* offsets, const int32_t* neighbours,
                                    int64_t n_entries, const uint8_t* pinned, double factor, float* out, p3d_stream_t stream)
{
    int rc = filter_sizes(n_vertices, n_entries, "mesh_smooth_step");
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(channels >= 1 && channels <= 256, "mesh_smooth_step: channels must be in [1, 256] (got %d)", channels);
    P3D_REQUIRE(isfinite(factor), "mesh_smooth_step: factor must be finite (got %g)", factor);
    if (n_vertices == 0) return P3D_OK;
    P3D_REQUIRE(x && out && offsets && (n_entries == 0 || neighbours), "mesh_smooth_step: null pointer");
    const int64_t total = (int64_t)n_vertices * channels;
    P3D_REQUIRE(!ranges_overlap(x, out, sizeof(float) * (size_t)total), "mesh_smooth_step: out overlaps x (a Jacobi step reads the old values)");
    hipLaunchKernelGGL(smooth_step_kernel, dim3(filter_grid(total, kNumCU * 16)), dim3(kFilterBlock), 0, (hipStream_t)stream, x, n_vertices,
                       channels, offsets, neighbours, n_entries, pinned, factor, out);
    count_launch(FAM_AUX);
    return check_launch("mesh_smooth_step");
}

extern "C" int p3d_mesh_label_vote(const uint8_t* labels, int32_t n_vertices, int32_t n_labels, const int64_t* offsets, const int32_t* neighbours,
                                   int64_t n_entries, const uint8_t* pinned, uint8_t* out, p3d_stream_t stream)
{
    int rc = filter_sizes(n_vertices, n_entries, "mesh_label_vote");
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(n_labels >= 1 && n_labels <= kVoteLabels, "mesh_label_vote: n_labels must be in [1, %d] (got %d)", kVoteLabels, n_labels);
    if (n_vertices == 0) return P3D_OK;
    P3D_REQUIRE(labels && out && offsets && (n_entries == 0 || neighbours), "mesh_label_vote: null pointer");
    P3D_REQUIRE(!ranges_overlap(labels, out, (size_t)n_vertices), "mesh_label_vote: out overlaps labels (the vote is synchronous)");
    const unsigned blocks = (unsigned)(((int64_t)n_vertices + kVoteBlock - 1) / kVoteBlock);
    hipLaunchKernelGGL(label_vote_kernel, dim3(blocks), dim3(kVoteBlock), 0, (hipStream_t)stream, labels, n_vertices, offsets, neighbours,
                       n_entries, pinned, out);
    count_launch(FAM_AUX);
    return check_launch("mesh_label_vote");
}

extern "C" int p3d_mesh_shade_smooth(const int32_t* face_id, const int32_t* proj, const float* vertices, int32_t n_vertices, const int32_t* faces,
                                     int32_t n_faces, const float* normals, const uint8_t* colors, const float* cameras, int32_t n_frames,
                                     int32_t orthographic, int32_t width, int32_t height, float ambient, int32_t bg_r, int32_t bg_g,
                                     int32_t bg_b, uint8_t* rgb, p3d_stream_t stream)
{
    (void)vertices;                                                       // (the operand list of p3d_mesh_shade; positions do not enter this shade)
    P3D_REQUIRE(n_vertices >= 0 && n_vertices < INT32_MAX, "mesh_shade_smooth: bad vertex count %d", n_vertices);
    P3D_REQUIRE(n_faces >= 0 && n_faces < INT32_MAX, "mesh_shade_smooth: bad face count %d", n_faces);
    P3D_REQUIRE(n_frames >= 0 && n_frames <= 65535, "mesh_shade_smooth: n_frames must be in [0, 65535] (got %d)", n_frames);
    P3D_REQUIRE(width >= 1 && height >= 1 && width <= 2048 && height <= 2048, "mesh_shade_smooth: image size %d x %d outside [1, 2048]^2",
                width, height);
    if (n_frames == 0) return P3D_OK;
    P3D_REQUIRE(face_id && cameras && rgb && (n_vertices == 0 || (proj && normals)) && (n_faces == 0 || faces), "mesh_shade_smooth: null pointer");
    hipLaunchKernelGGL(mesh_shade_smooth_kernel, dim3(filter_grid((int64_t)n_frames * width * height, kNumCU * 16)), dim3(kFilterBlock), 0,
                       (hipStream_t)stream, face_id, (const int4*)proj, n_vertices, faces, n_faces, normals, colors, cameras, n_frames,
                       orthographic, width, height, ambient, bg_r & 255, bg_g & 255, bg_b & 255, rgb);
    count_launch(FAM_AUX);
    return check_launch("mesh_shade_smooth");
}
