// Mesh clean-up for gfx950: connected components and vertex-clustering decimation (include/p3d_hip.h; pix2pix3d_amd/mesh.py).
//
// p3d_mesh_components: union-find in the ECL-CC shape (Jaiganesh & Burtscher, HPDC 2018): init, hook, flatten, three launches whatever
// the mesh.  parent[] lives in the output array.  The protocol (what a hook, a find and a failed CAS may do, and why no lane waits on
// another) is stated with the functions, in csrc/union_find.h.
//
// p3d_mesh_cluster_keys / _means / _faces: the three kernels of mesh.simplify.  Plain gathers and stores, one thread per vertex,
// cluster or face; the sums of _means run in a fixed order in fp64, so the output is a pure function of the inputs.
#include "p3d_common.h"
#include "union_find.h"
#include <math.h>

namespace p3d {

constexpr int kMeshOpsBlock = 256;

__global__ void __launch_bounds__(kMeshOpsBlock) cc_init_kernel(int32_t* __restrict__ parent, int32_t nv)
{
    const int64_t v = (int64_t)blockIdx.x * kMeshOpsBlock + threadIdx.x;
    if (v < nv) parent[v] = (int32_t)v;
}

__global__ void __launch_bounds__(kMeshOpsBlock) cc_hook_kernel(const int32_t* __restrict__ faces, int32_t nf, int32_t nv, int32_t* parent)
{
    const int64_t t = (int64_t)blockIdx.x * kMeshOpsBlock + threadIdx.x;
    if (t >= nf) return;
    const int32_t a = faces[t * 3], b = faces[t * 3 + 1], c = faces[t * 3 + 2];
    if ((unsigned)a >= (unsigned)nv || (unsigned)b >= (unsigned)nv || (unsigned)c >= (unsigned)nv) return;
    uf_union(parent, a, b);                                          // (a, c) follows from the other two
    uf_union(parent, b, c);
}

__global__ void __launch_bounds__(kMeshOpsBlock) cc_flatten_kernel(int32_t* parent, int32_t nv)
{
    const int64_t v = (int64_t)blockIdx.x * kMeshOpsBlock + threadIdx.x;
    if (v >= nv) return;
    int32_t cur = uf_load(parent + v), next;
    while (cur > (next = uf_load(parent + cur))) cur = next;
    uf_store(parent + v, cur);                                       // readers that race with this see the old parent or the root: both ancestors
}

// ---- vertex clustering ---------------------------------------------------------------------------------------
struct ClusterGrid { float lo[3]; double cell; int32_t n[3]; };

__device__ __forceinline__ int64_t cluster_axis(float x, float lo, double cell, int32_t n)
{
    const double q = floor(((double)x - (double)lo) / cell);         // a subtract and a divide: nothing to contract
    return (int64_t)fmin(fmax(q, 0.0), (double)(n - 1));             // (NaN -> 0; the Python layer rejects non-finite vertices)
}

__global__ void __launch_bounds__(kMeshOpsBlock) cluster_keys_kernel(const float* __restrict__ vertices, int32_t nv, ClusterGrid g,
                                                                     int64_t* __restrict__ key)
{
    const int64_t v = (int64_t)blockIdx.x * kMeshOpsBlock + threadIdx.x;
    if (v >= nv) return;
    const int64_t ix = cluster_axis(vertices[v * 3], g.lo[0], g.cell, g.n[0]);
    const int64_t iy = cluster_axis(vertices[v * 3 + 1], g.lo[1], g.cell, g.n[1]);
    const int64_t iz = cluster_axis(vertices[v * 3 + 2], g.lo[2], g.cell, g.n[2]);
    key[v] = (iz * g.n[1] + iy) * g.n[0] + ix;
}

__global__ void __launch_bounds__(kMeshOpsBlock) cluster_means_kernel(const float* __restrict__ vertices, int32_t nv,
                                                                      const int32_t* __restrict__ order, const int64_t* __restrict__ offsets,
                                                                      int32_t nc, float* __restrict__ means)
{
    const int64_t c = (int64_t)blockIdx.x * kMeshOpsBlock + threadIdx.x;
    if (c >= nc) return;
    int64_t s = offsets[c], e = offsets[c + 1];
    s = s < 0 ? 0 : s;
    e = e > nv ? nv : e;
    double x = 0.0, y = 0.0, z = 0.0;
    int64_t m = 0;
    for (int64_t k = s; k < e; ++k) {                                // ascending vertex id: `order` is a stable sort by key
        const int32_t v = order[k];
        if ((unsigned)v >= (unsigned)nv) continue;
        x += (double)vertices[(int64_t)v * 3];
        y += (double)vertices[(int64_t)v * 3 + 1];
        z += (double)vertices[(int64_t)v * 3 + 2];
        ++m;
    }
    const double d = (double)(m > 0 ? m : 1);
    means[c * 3] = (float)(x / d);
    means[c * 3 + 1] = (float)(y / d);
    means[c * 3 + 2] = (float)(z / d);
}

__global__ void __launch_bounds__(kMeshOpsBlock) cluster_faces_kernel(const int32_t* __restrict__ faces, int32_t nf, int32_t nv,
                                                                      const int32_t* __restrict__ cluster, int32_t* __restrict__ mapped,
                                                                      int32_t* __restrict__ sorted, uint8_t* __restrict__ degenerate)
{
    const int64_t t = (int64_t)blockIdx.x * kMeshOpsBlock + threadIdx.x;
    if (t >= nf) return;
    const int32_t a = faces[t * 3], b = faces[t * 3 + 1], c = faces[t * 3 + 2];
    const bool ok = (unsigned)a < (unsigned)nv && (unsigned)b < (unsigned)nv && (unsigned)c < (unsigned)nv;
    const int32_t ca = ok ? cluster[a] : 0, cb = ok ? cluster[b] : 0, cc = ok ? cluster[c] : 0;
    mapped[t * 3] = ca; mapped[t * 3 + 1] = cb; mapped[t * 3 + 2] = cc;
    const int32_t lo = min(ca, min(cb, cc)), hi = max(ca, max(cb, cc));
    const int32_t mid = max(min(ca, cb), min(max(ca, cb), cc));
    sorted[t * 3] = lo; sorted[t * 3 + 1] = mid; sorted[t * 3 + 2] = hi;
    degenerate[t] = (uint8_t)(!ok || ca == cb || cb == cc || ca == cc);
}

static int mesh_ops_sizes(int32_t n_faces, int32_t n_vertices, const char* what)
{
    P3D_REQUIRE(n_faces >= 0 && n_vertices >= 0, "%s: negative size (%d faces, %d vertices)", what, n_faces, n_vertices);
    if (n_faces > INT32_MAX - 1 || n_vertices > INT32_MAX - 1)
        return fail(P3D_ERR_UNSUPPORTED, "%s: at most INT32_MAX - 1 faces and vertices (got %d, %d)", what, n_faces, n_vertices);
    return P3D_OK;
}

static inline unsigned mesh_ops_blocks(int64_t n) { return (unsigned)((n + kMeshOpsBlock - 1) / kMeshOpsBlock); }

} // namespace p3d

using namespace p3d;

extern "C" int p3d_mesh_components(const int32_t* faces, int32_t n_faces, int32_t n_vertices, int32_t* label, p3d_stream_t stream)
{
    int rc = mesh_ops_sizes(n_faces, n_vertices, "mesh_components");
    if (rc != P3D_OK) return rc;
    if (n_vertices == 0) return P3D_OK;
    P3D_REQUIRE(label && (n_faces == 0 || faces), "mesh_components: null pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_init_kernel, dim3(mesh_ops_blocks(n_vertices)), dim3(kMeshOpsBlock), 0, s, label, n_vertices);
    count_launch(FAM_AUX);
    rc = check_launch("mesh_components_init");
    if (rc != P3D_OK || n_faces == 0) return rc;
    hipLaunchKernelGGL(cc_hook_kernel, dim3(mesh_ops_blocks(n_faces)), dim3(kMeshOpsBlock), 0, s, faces, n_faces, n_vertices, label);
    count_launch(FAM_AUX);
    rc = check_launch("mesh_components_hook");
    if (rc != P3D_OK) return rc;
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(mesh_ops_blocks(n_vertices)), dim3(kMeshOpsBlock), 0, s, label, n_vertices);
    count_launch(FAM_AUX);
    return check_launch("mesh_components_flatten");
}

extern "C" int p3d_mesh_cluster_keys(const float* vertices, int32_t n_vertices, float lo_x, float lo_y, float lo_z, double cell,
                                     int32_t nx, int32_t ny, int32_t nz, int64_t* key, p3d_stream_t stream)
{
    int rc = mesh_ops_sizes(0, n_vertices, "mesh_cluster_keys");
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(cell > 0.0 && isfinite(cell), "mesh_cluster_keys: cell must be positive and finite (got %g)", cell);
    P3D_REQUIRE(isfinite(lo_x) && isfinite(lo_y) && isfinite(lo_z), "mesh_cluster_keys: lo must be finite");
    P3D_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "mesh_cluster_keys: bad cell counts %d x %d x %d", nx, ny, nz);
    if ((int64_t)nx * ny > (((int64_t)1 << 62) - 1) / nz)            // nx * ny < 2^62 itself: both are below 2^31
        return fail(P3D_ERR_UNSUPPORTED, "mesh_cluster_keys: %d x %d x %d cells do not fit a key below 2^62", nx, ny, nz);
    if (n_vertices == 0) return P3D_OK;
    P3D_REQUIRE(vertices && key, "mesh_cluster_keys: null pointer");
    const ClusterGrid g{{lo_x, lo_y, lo_z}, cell, {nx, ny, nz}};
    hipLaunchKernelGGL(cluster_keys_kernel, dim3(mesh_ops_blocks(n_vertices)), dim3(kMeshOpsBlock), 0, (hipStream_t)stream, vertices,
                       n_vertices, g, key);
    count_launch(FAM_AUX);
    return check_launch("mesh_cluster_keys");
}

extern "C" int p3d_mesh_cluster_means(const float* vertices, int32_t n_vertices, const int32_t* order, const int64_t* offsets,
                                      int32_t n_clusters, float* means, p3d_stream_t stream)
{
    int rc = mesh_ops_sizes(0, n_vertices, "mesh_cluster_means");
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(n_clusters >= 0 && n_clusters <= n_vertices, "mesh_cluster_means: %d clusters for %d vertices", n_clusters, n_vertices);
    if (n_clusters == 0) return P3D_OK;
    P3D_REQUIRE(vertices && order && offsets && means, "mesh_cluster_means: null pointer");
    hipLaunchKernelGGL(cluster_means_kernel, dim3(mesh_ops_blocks(n_clusters)), dim3(kMeshOpsBlock), 0, (hipStream_t)stream, vertices,
                       n_vertices, order, offsets, n_clusters, means);
    count_launch(FAM_AUX);
    return check_launch("mesh_cluster_means");
}

extern "C" int p3d_mesh_cluster_faces(const int32_t* faces, int32_t n_faces, int32_t n_vertices, const int32_t* cluster, int32_t* mapped,
                                      int32_t* sorted, uint8_t* degenerate, p3d_stream_t stream)
{
    int rc = mesh_ops_sizes(n_faces, n_vertices, "mesh_cluster_faces");
    if (rc != P3D_OK) return rc;
    if (n_faces == 0) return P3D_OK;
    P3D_REQUIRE(faces && mapped && sorted && degenerate && (n_vertices == 0 || cluster), "mesh_cluster_faces: null pointer");
    hipLaunchKernelGGL(cluster_faces_kernel, dim3(mesh_ops_blocks(n_faces)), dim3(kMeshOpsBlock), 0, (hipStream_t)stream, faces, n_faces,
                       n_vertices, cluster, mapped, sorted, degenerate);
    count_launch(FAM_AUX);
    return check_launch("mesh_cluster_faces");
}
