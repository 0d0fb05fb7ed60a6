/* libp3d_mesh.so — quadric-error mesh decimation (csrc/mesh/mesh_decimate.hip; pix2pix3d_amd/decimate.py).  A library of its
 * own, like libp3d_regions.so: the product ABI (include/p3d_hip.h, libp3d_hip.so) exports none of this.  It carries its own copy of the library
 * services (p3d_last_error, p3d_launch_count).  All pointers are device memory.  Argument errors return P3D_ERR_ARGUMENT before any launch.
 *
 * Quadric-error decimation by ROUNDS of edge collapses: every round rates every edge of the current mesh, picks a set of cheap edges no two
 * of which touch each other's 1-rings, and collapses them at once.  The four entry points below are the device half of a round; the sorts
 * and scans between them (mesh.adjacency, the vertex -> face list, the ranks) are torch on the tensors' device (decimate.py).
 *
 * The mesh: vertices float32 [V][3]; faces int32 [T][3], indices in [0, V) (an entry that is not is skipped, never followed); counts below
 * P3D_MESH_DECIMATE_MAX.  Vertices are never renumbered between rounds: V is the input's.  Lists are CSR: the list of v is
 * list[offsets[v] .. offsets[v + 1]), offsets int64 [V + 1], clamped to the list's length.
 *     adjacency      (adj_offsets, neighbours int32 [n_entries]): mesh.adjacency's, ascending ids inside a list.
 *     vertex -> face (vf_offsets, vf_faces int32 [3 T]): the corners f * 3 + k sorted by their vertex with a stable sort; vf_faces holds
 *                    the face f of every corner, so a list is in ascending face id (a face that names v twice is in v's list twice).
 *     edges          int32 [E][2] = (a, b), a < b: the distinct undirected pairs in ascending a * V + b; the rank in that list is the edge id.
 *
 * Arithmetic: fp64 from the float32 positions, every operator rounded once (no contraction), in exactly the order written here:
 *     u - v, componentwise;   u . v = ((u0 v0) + u1 v1) + u2 v2;   u x v = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0);
 *     the normal of a face (a, b, c) is n = (b - a) x (c - a).
 * A position is rounded to fp32 once, when a vertex moves.
 *
 * 1. Quadrics, once, from the input mesh.  A face with n . n == 0 adds nothing.  Otherwise l = sqrt(n . n), h = n / l (three divisions),
 *    p = (h0, h1, h2, -(h . a)), w = l * 0.5, and the face adds K[k] = w * (p_r * p_c) for the ten pairs r <= c in the order
 *    k = (00, 01, 02, 03, 11, 12, 13, 22, 23, 33).  Q[v] float64 [10] is the sum of K over v's vertex -> face list, in list order, from +0.
 *
 * 2. An edge (a, b) is VALID when all of these hold:
 *    - fixed[a] == 0 and fixed[b] == 0 (the caller ORs the boundary flags of mesh.adjacency and the pinned vertices into `fixed`);
 *    - exactly two entries of a's vertex -> face list are faces with b as a corner; the third corner of such a face is its first corner
 *      that is neither a nor b (its last corner if there is none); the two third corners t0, t1 differ;
 *    - the merge of the two ascending neighbour lists finds exactly two common neighbours, the smaller one min(t0, t1) and the larger one
 *      max(t0, t1) (the link condition), and each of them has at least 4 neighbours (a tetrahedron must not fold flat);
 *    - the merged vertex keeps at least 4 neighbours: (neighbours of a) + (neighbours of b) - 4 >= 4 (an octahedron stops at the 6 faces of a
 *      bipyramid and is not folded on into a tetrahedron);
 *    - the cost below is finite;
 *    - the flip test: for every entry of a's list whose face does not use b, and every entry of b's list whose face does not use a, with
 *      n0 the face's normal, n0 . n0 > 0, and n1 its normal with the corners equal to that end replaced by the TARGET (the fp32 point
 *      below, widened): d = n0 . n1 > 0 and d * d >= ((n0 . n0) * (n1 . n1)) * 0.0625.
 *
 * 3. Target point and cost.  q = Q[a] + Q[b] (ten additions).  For a point x,
 *        r0 = ((q0 x0 + q1 x1) + q2 x2) + q3,  r1 = ((q1 x0 + q4 x1) + q5 x2) + q6,  r2 = ((q2 x0 + q5 x1) + q7 x2) + q8,
 *        r3 = ((q3 x0 + q6 x1) + q8 x2) + q9,  c = ((x0 r0 + x1 r1) + x2 r2) + r3,   cost(x) = c > 0 ? c : 0.
 *    Candidates in this order: V[a], V[b], mid = (V[a] + V[b]) * 0.5, and the minimiser s of q by cofactors:
 *        c00 = q4 q7 - q5 q5,  c01 = q2 q5 - q1 q7,  c02 = q1 q5 - q2 q4,  c11 = q0 q7 - q2 q2,  c12 = q1 q2 - q0 q5,  c22 = q0 q4 - q1 q1,
 *        det = (q0 c00 + q1 c01) + q2 c02,   m = the largest of |q0|, |q1|, |q2|, |q4|, |q5|, |q7|,
 *        s = (-((c00 q3 + c01 q6) + c02 q8) / det,  -((c01 q3 + c11 q6) + c12 q8) / det,  -((c02 q3 + c12 q6) + c22 q8) / det),
 *    which is a candidate only if |det| > ((m m) m) 2^-20 and (s - mid) . (s - mid) <= ((V[b] - V[a]) . (V[b] - V[a])) * 4.  The smallest
 *    cost wins and a tie goes to the earlier candidate, so that a flat region never moves a vertex off its surface.  target = the winner
 *    rounded to fp32.  An edge that is not valid gets target (0, 0, 0), cost +inf and valid 0.
 *
 * 4. Order and candidates (torch).  The valid edges are ranked by (cost, mix(edge id)), mix being the 32-bit bijection
 *    x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15, x *= 0x846ca68b, x ^= x >> 16: a tie broken by the plain id lets a flat region hold one
 *    local minimum and a round one collapse.  With T the faces, need = ceil((T - target_faces) / 2) and k = min(max(1, ceil(fraction *
 *    valid)), need), the CANDIDATES are the valid edges with cost <= the cost at rank k - 1 (ties included whole).  rank int32 [E] holds a
 *    candidate's rank and P3D_MESH_NO_RANK for every other edge.
 *
 * 5. Independent set.  m1[v] = the smallest rank among the edges of v (entry_edge int32 [n_entries]: the edge id of every adjacency entry);
 *    m2[v] = the minimum of m1 over v and its neighbours; an edge WINS when its rank is not P3D_MESH_NO_RANK and equals m2[a] and m2[b].
 *    No two winners touch each other's 1-rings, so every test of 2. still holds when they are applied together, and the smallest candidate
 *    always wins.  Of the winners the `need` lowest ranks are APPLIED (torch).
 *
 * 6. Collapse.  For an applied edge: V[a] = target, Q[a] = Q[a] + Q[b], parent[b] = a.  Then every face corner x becomes parent[x], and a
 *    face with two equal corners is flagged dead.  The caller compacts the faces (stably) and, once at the end, the vertices.          */
#ifndef P3D_MESH_H
#define P3D_MESH_H
#include <stdint.h>
#include "../../../include/p3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define P3D_MESH_QUADRIC_DOUBLES 10
#define P3D_MESH_DECIMATE_MAX 1073741824         /* 2^30: every count is below it */
#define P3D_MESH_NO_RANK 2147483647

/* Rule 1.  quadrics float64 [V][10], 8-byte aligned.  n_vertices == 0 is a success that launches nothing.  One launch, a thread per vertex. */
int p3d_mesh_quadrics(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces, const int64_t* vf_offsets,
                      const int32_t* vf_faces, double* quadrics, p3d_stream_t stream);

/* Rules 2 and 3.  fixed uint8 [V]; target float32 [E][3], cost float64 [E], valid uint8 [E].  n_edges == 0 is a success that launches
 * nothing.  One launch, a thread per edge.                                                                                              */
int p3d_mesh_edge_costs(const float* vertices, const double* quadrics, int32_t n_vertices, const int32_t* faces, int32_t n_faces,
                        const int64_t* adj_offsets, const int32_t* neighbours, int64_t n_entries, const uint8_t* fixed,
                        const int64_t* vf_offsets, const int32_t* vf_faces, const int32_t* edges, int32_t n_edges, float* target,
                        double* cost, uint8_t* valid, p3d_stream_t stream);

/* Rule 5.  m1, m2 int32 [V]: two workspaces that hold m1 and m2 afterwards; win uint8 [E].  Three launches: a thread per vertex twice,
 * then a thread per edge.                                                                                                                */
int p3d_mesh_edge_select(const int32_t* rank, const int32_t* edges, int32_t n_edges, int32_t n_vertices, const int64_t* adj_offsets,
                         const int32_t* neighbours, const int32_t* entry_edge, int64_t n_entries, int32_t* m1, int32_t* m2, uint8_t* win,
                         p3d_stream_t stream);

/* Rule 6, in place on vertices, quadrics, parent int32 [V] and faces; apply uint8 [E]; dead uint8 [T].  Applied edges must share no vertex
 * (rule 5 sees to it).  Two launches: a thread per edge, then a thread per face (one launch when n_edges == 0).                          */
int p3d_mesh_collapse(float* vertices, double* quadrics, int32_t* parent, int32_t n_vertices, int32_t* faces, int32_t n_faces,
                      const int32_t* edges, const uint8_t* apply, const float* target, int32_t n_edges, uint8_t* dead, p3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
