/*
 * p3d_mesh_distance.h — mesh-to-mesh distances: surface samples, a bounding-volume hierarchy over the faces and the closest-triangle
 * query (csrc/mesh_distance.hip; pix2pix3d_amd/geometry.py).  The kernels are part of libp3d_hip.so and count in its launch counter
 * (family 5, like every mesh kernel); geometry.py binds these prototypes onto the loaded library.  They are declared here and not in
 * include/p3d_hip.h because the set of prototypes of that header is pinned (tests/golden/abi_signatures_parent.json).
 *
 * Meshes are indexed as in "mesh clean-up" of p3d_hip.h: vertices float32 [V][3], faces int32 [T][3], V and T <= INT32_MAX - 1
 * (P3D_ERR_UNSUPPORTED beyond).  A face is VALID when its three indices lie in [0, V) and its nine coordinates are finite; every
 * kernel here skips the others.  All arithmetic below is fp64 on the fp32 inputs with one rounding per operator and no contraction
 * (#pragma clang fp contract(off), as in csrc/mesh_tri.h), so that torch's element-wise fp64 ops reproduce it bit for bit: the CPU
 * formulation of geometry.py is the definition and the kernels' bytes equal it.  For u, v in R^3:
 *     dot(u, v)   = u0 v0;  + u1 v1;  + u2 v2          (every product rounded, summed left to right)
 *     cross(u, v) = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0)      (both products rounded, then the difference)
 * and a difference of two points is taken per component in fp64 (one rounding).
 *
 * ---- surface samples ----------------------------------------------------------------------------------------------------------
 * p3d_mesh_sample_counts: k int32 [T] <- the subdivision count of every face, 0 for a face that is not valid; capped uint8 [T] <- 1
 *   where the face wanted more than k_max.  With L2 the largest of the three squared edge lengths dot(e, e), e = b - a, c - b, a - c,
 *   and s2 = spacing^2 (computed once by the caller in fp64, > 0 and finite), k is the smallest integer in [1, k_max] with
 *       (double)(k k) s2 >= L2
 *   (k k an exact integer, one rounded product), or k_max when there is none; 1 <= k_max <= P3D_MESH_SAMPLE_KMAX.  Found by bisection on
 *   the predicate, which is monotone in k: no square root decides an integer.
 * p3d_mesh_sample_points: the face contributes k^2 points, the centroids of its k^2 congruent sub-triangles.  offsets int64 [T + 1] is
 *   the exclusive sum of k^2 over the faces (the caller's cumsum; offsets[T] = N <= INT32_MAX - 1).  Point n belongs to the face f with
 *   offsets[f] <= n < offsets[f + 1]; with r = n - offsets[f]: the first k (k + 1) / 2 are the upright sub-triangles (i, j), i + j <= k - 1,
 *   i outer and j inner, both ascending, with barycentric numerators over 3 k of (n0, n1, n2) = (3 i + 1, 3 j + 1, 3 k - n0 - n1); the
 *   k (k - 1) / 2 inverted ones (i, j), i + j <= k - 2, follow in the same order with (3 i + 2, 3 j + 2, 3 k - n0 - n1).  Per component,
 *   with a_c the face's corner c:   s = n0 a_0;  s = s + n1 a_1;  s = s + n2 a_2;  s / (3 k), rounded to fp32
 *   (the arithmetic of p3d_mesh_atlas_texels).  points float32 [N][3], face int32 [N].  Two launches with the caller's scan between them.
 *
 * ---- point-to-triangle distance -----------------------------------------------------------------------------------------------
 * tri_d2(p; a, b, c), the squared distance from p to the closed triangle; total for finite inputs (a face with two equal corners is
 * its segment, with three a point), never a NaN, and every division stands behind a test that its denominator is positive:
 *     seg(p; a, b):  e = b - a;  r = p - a;  den = dot(e, e);  num = dot(r, e);  t = den > 0 ? num / den : 0;  t = min(max(t, 0), 1);
 *                    q_k = r_k - t e_k;  seg = dot(q, q)
 *     s  = min(min(seg(p; a, b), seg(p; b, c)), seg(p; c, a))
 *     e1 = b - a;  e2 = c - a;  n = cross(e1, e2);  nn = dot(n, n);  ra = p - a;  rb = p - b;  rc = p - c
 *     wc = dot(cross(e1, ra), n);  wa = dot(cross(c - b, rb), n);  wb = dot(cross(a - c, rc), n)
 *     h  = dot(ra, n);  plane = (nn > 0 and wa >= 0 and wb >= 0 and wc >= 0) ? (h h) / nn : s;  m = min(s, plane)
 *     lo_k = min(a_k, b_k, c_k);  hi_k = max(a_k, b_k, c_k);  g_k = max(max(lo_k - p_k, p_k - hi_k), 0);  box = dot(g, g)
 *     tri_d2 = max(m, box)
 *   The last line costs nothing in accuracy (the true distance to a triangle is never below the distance to its bounding box, so it
 *   only lifts an underestimate that rounding made, e.g. of the plane term of a sliver) and is what makes the tree below exact: box
 *   is the SAME expression the query evaluates for a node's box, it is monotone in lo and hi under rounding, and a node's box contains
 *   the boxes of its faces, so box(node) <= box(face) <= tri_d2(p; face) holds for the COMPUTED values, with no appeal to error bounds.
 * closest: d2[n] = the minimum of tri_d2 over the valid faces, face[n] = the smallest face id that attains it; (+inf, -1) for a point
 *   with a non-finite coordinate and for every point when no face is valid.
 *
 * ---- the hierarchy ---------------------------------------------------------------------------------------------------------------
 * p3d_mesh_bvh_keys: key int64 [n_items] <- a 63-bit Morton key.  box float32 [6] = (lo, hi) of the finite vertices, on the device (the
 *   caller's reduction).  Item t is face t (its corner sum c_k = (a_k + b_k) + c_k) or, with faces NULL, vertex t taken three times (a
 *   query point sorts like a face at that point).  Per axis x_k = floor((c_k - 3 lo_k) / (3 (hi_k - lo_k)) 2^21) clamped to
 *   [0, 2^21 - 1], 0 where the extent is not positive; bit b of x_k goes to bit 3 b + k.  An item that is not valid gets INT64_MAX.  The
 *   keys only order the items: no result depends on them.
 * The caller sorts the face ids STABLY by key -> order int32 [T].  Leaf l holds the P3D_MESH_BVH_LEAF consecutive sorted faces
 *   order[l LEAF .. (l + 1) LEAF); n_leaves = ceil(T / LEAF), padded to n_pad, the next power of two (>= 1).  The tree is the implicit
 *   complete binary tree of 2 n_pad - 1 nodes in heap order (children of i: 2 i + 1, 2 i + 2; leaf l is node n_pad - 1 + l).
 * p3d_mesh_bvh_build: tris float32 [n_leaves LEAF][12] <- per sorted slot the corners a, b, c as three float4 whose first w holds the
 *   face id as int32 bits (-1: the face is not valid, or the slot lies beyond T); nodes float32 [2 n_pad - 1][8] <- (lo.xyz, -, hi.xyz, -)
 *   per node: the min / max of fp32 values, exact and order-independent; (+inf, -inf) for a node without valid faces.  One launch for
 *   the leaves, then one per level, bottom up: no work-group reads what another wrote in the same launch, so there are no flags,
 *   counters or spins.
 * p3d_mesh_closest: one point per lane; a stack of node ids in LDS (one column per lane, depth + 1 <= 32 rows, sized by the launch).
 *   At an inner node both children's box distances are computed, the farther is pushed and the nearer entered; a node is entered or
 *   pushed only if NOT box (1 - 2^-P3D_MESH_BVH_MARGIN_LOG2) > best, and tested again when popped.  By the inequality above pruning
 *   without any margin is already exact for the computed values; the margin (2^-20, far above the 2^-52 of fp64) is kept so that
 *   the property does not hang on that argument alone.  Ties go to the smaller face id and equal box bounds are entered, so the
 *   result is the definition's, bit for bit, whatever the traversal order.  The loop visits every node at most once; it counts its
 *   iterations and, past the node count (or on a full stack), stores 1 to status int32 [1] (zeroed by the caller) and gives (+inf, -2)
 *   instead of running on: the caller reports P3D_ERR_LAUNCH.  d2 double [N], face int64 [N].
 */
#ifndef P3D_MESH_DISTANCE_H
#define P3D_MESH_DISTANCE_H

#include "../../include/p3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P3D_MESH_SAMPLE_KMAX 1024
#define P3D_MESH_BVH_LEAF 4
#define P3D_MESH_BVH_MARGIN_LOG2 20
#define P3D_MESH_BVH_MAX_DEPTH 31

int p3d_mesh_sample_counts(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces, double spacing2,
                           int32_t k_max, int32_t* k, uint8_t* capped, p3d_stream_t stream);
int p3d_mesh_sample_points(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces, const int32_t* k,
                           const int64_t* offsets, int64_t n_points, float* points, int32_t* face, p3d_stream_t stream);
int p3d_mesh_bvh_keys(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_items, const float* box,
                      int64_t* key, p3d_stream_t stream);
int p3d_mesh_bvh_build(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces, const int32_t* order,
                       int32_t n_pad, float* tris, float* nodes, p3d_stream_t stream);
int p3d_mesh_closest(const float* points, int64_t n_points, const float* tris, const float* nodes, int32_t n_faces, int32_t n_pad,
                     double* d2, int64_t* face, int32_t* status, p3d_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
