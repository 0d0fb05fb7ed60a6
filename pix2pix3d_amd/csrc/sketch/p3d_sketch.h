/* libp3d_sketch.so — the edge-map canvas of a sketch session (pix2pix3d_amd/sketch.py): ink to the Encoder's conditioning
 * image, edges from a picture, hysteresis, thinning.  A library of its own, like libp3d_regions.so: the product ABI (include/p3d_hip.h,
 * libp3d_hip.so) exports none of this.  It carries its own copy of the library services (p3d_last_error, p3d_launch_count).
 *
 * Every image is uint8 [h][w], pixels contiguous, rows `*_row_pitch` bytes apart (>= w; >= 3 w for RGB); 1 <= h, w <= P3D_PAINT_MAX_SIZE.  Every
 * result is written out of place and is a pure function of the inputs: the torch formulations of pix2pix3d_amd/sketch.py produce the same bytes.
 * All pointers are device memory.  Argument errors return P3D_ERR_ARGUMENT before any launch.
 *
 * REFLECT: a tap at index i of an axis of n pixels reads the index after three steps in this order: if i < 0, i = -i; if i >= n,
 * i = 2 n - 2 - i; i = min(max(i, 0), n - 1)  (reflect-101; the clamp keeps it defined for n = 1 and n = 2).  All arithmetic is in 32-bit
 * integers.                                                                                                                                */
#ifndef P3D_SKETCH_H
#define P3D_SKETCH_H
#include <stdint.h>
#include "../../../include/p3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define P3D_SKETCH_MAX_MAGNITUDE 2040     /* |gx| + |gy| of the 3 x 3 Sobel pair on 8-bit values: 4 * 255 each */
#define P3D_SKETCH_TILE_W 64              /* the work-group tile of p3d_sketch_edge_classes (tests straddle it) */
#define P3D_SKETCH_TILE_H 16

/* Ink canvas (255 = full ink, 0 = paper) -> the Encoder's conditioning image, float32 [resolution][resolution], rows `out_row_pitch` FLOATS
 * apart (>= resolution).  For the output pixel (x, y):
 *     sy = min(y * h / resolution, h - 1),  sx = min(x * w / resolution, w - 1)                     (integer division: a nearest resize)
 *     m  = blur ? (sum of the nine REFLECT taps of ink about (sx, sy) + 4) / 9 : ink[sy][sx]        (the 3 x 3 box blur, at the sampled pixel only)
 *     out[y][x] = table[m]                                                                          (table float32 [256])
 * 1 <= resolution <= P3D_PAINT_MAX_SIZE.  One launch.                                                                                     */
int p3d_sketch_condition(const uint8_t* ink, int64_t ink_row_pitch, int32_t h, int32_t w, int32_t blur, const float* table, float* out,
                         int64_t out_row_pitch, int32_t resolution, p3d_stream_t stream);

/* A frame -> edge classes uint8 [h][w]: 0 none, 1 weak, 2 strong.  `channels` 3: image is RGB uint8 [h][w][3] (row pitch >= 3 w);
 * `channels` 1: grey uint8 [h][w].  0 <= low <= high <= P3D_SKETCH_MAX_MAGNITUDE.
 *   1. luma    g = (77 r + 150 g + 29 b + 128) >> 8                                  (a grey frame is g itself)
 *   2. smooth  (if `smooth`) v = sum over i, j in -2 .. 2 of k[i] k[j] g[REFLECT(y + i)][REFLECT(x + j)], k = [1 4 6 4 1] — the separable
 *              filter, rounded once after both passes: s = (v + 128) >> 8; otherwise s = g
 *   3. Sobel   on REFLECT taps of s:  gx = (s[y-1][x+1] + 2 s[y][x+1] + s[y+1][x+1]) - (s[y-1][x-1] + 2 s[y][x-1] + s[y+1][x-1]),
 *              gy = (s[y+1][x-1] + 2 s[y+1][x] + s[y+1][x+1]) - (s[y-1][x-1] + 2 s[y-1][x] + s[y-1][x+1]);  mag = |gx| + |gy|
 *   4. non-maximum suppression; mag OUTSIDE the image counts as 0.  ax = |gx|, ay = |gy| << 15, t22 = ax * 13573, t67 = t22 + (ax << 16)
 *              (tan 22.5 degrees in 15-bit fixed point):
 *                  ay < t22:   keep iff mag > mag[y][x-1] && mag >= mag[y][x+1]
 *                  ay > t67:   keep iff mag > mag[y-1][x] && mag >= mag[y+1][x]
 *                  otherwise,  s = ((gx ^ gy) < 0) ? -1 : 1:  keep iff mag > mag[y-1][x-s] && mag > mag[y+1][x+s]
 *   5. class   kept && mag > high ? 2 : (kept && mag > low ? 1 : 0)
 * ONE launch: a work-group owns P3D_SKETCH_TILE_W x P3D_SKETCH_TILE_H pixels and keeps the grey tile with its halo, the smoothed tile and the
 * gradients of the tile and its one-pixel halo in LDS; global memory is read once per tile.                                                */
int p3d_sketch_edge_classes(const uint8_t* image, int64_t image_row_pitch, int32_t channels, uint8_t* classes, int64_t classes_row_pitch,
                            int32_t h, int32_t w, int32_t low, int32_t high, int32_t smooth, p3d_stream_t stream);

/* Hysteresis.  classes: the class map; ids int32 [h][w], contiguous: p3d_label_components (libp3d_regions.so) of the byte map classes != 0
 * under the 8-neighbourhood, so ids[p] is a linear index inside [0, h w).  flag: int32 [h * w] workspace.
 *     ink[p] = classes[p] != 0 && the component of p holds a class-2 pixel ? 255 : 0.
 * The workspace is cleared by a memset on the stream, then TWO launches: mark (every class-2 pixel stores 1 to flag[ids[p]]: plain vector
 * stores of one value, whatever their order) and select (reads flag[ids[p]]).  An id outside [0, h w) is never followed.                 */
int p3d_sketch_link(const uint8_t* classes, int64_t classes_row_pitch, const int32_t* ids, int32_t* flag, uint8_t* ink, int64_t ink_row_pitch,
                    int32_t h, int32_t w, p3d_stream_t stream);

/* One parallel Zhang-Suen sub-iteration.  A pixel is SET iff src >= threshold (1 <= threshold <= 255).  Its neighbour code has bit i set for the
 * set neighbour i of N, NE, E, SE, S, SW, W, NW (outside the image: unset).  With B = the number of set neighbours and A = the number of unset -> set
 * steps around the cycle N, NE, .., NW, N a code is DELETABLE in step 0 iff 2 <= B <= 6, A == 1, N E S == 0 and E S W == 0, and in step 1 iff
 * 2 <= B <= 6, A == 1, N E W == 0 and N S W == 0 (csrc/sketch/thin_table.h, generated by pix2pix3d_amd/sketch.py).
 *     dst = set && !deletable[step][code] ? 255 : 0.         step is 0 or 1; dst must not be src.  One launch.                              */
int p3d_sketch_thin_step(const uint8_t* src, int64_t src_row_pitch, uint8_t* dst, int64_t dst_row_pitch, int32_t h, int32_t w, int32_t threshold,
                         int32_t step, p3d_stream_t stream);

/* ---- mesh decimation (csrc/sketch/mesh_decimate.hip; pix2pix3d_amd/decimate.py) --------------------------------------
 * Quadric-error decimation by ROUNDS of edge collapses: every round rates every edge of the current mesh, picks a set of cheap edges no two
 * of which touch each other's 1-rings, and collapses them at once.  The four entry points below are the device half of a round; the sorts
 * and scans between them (mesh.adjacency, the vertex -> face list, the ranks) are torch on the tensors' device (decimate.py).
 *
 * Why here: the product header, the set of side libraries and the prototype lists of the regions and video headers are each pinned by tests, and a new
 * library would need a row of its own; this library's header is the one that may grow.  Nothing below touches a sketch.
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

/* ---- multi-scale frame quality (csrc/sketch/frame_multiscale.hip; pix2pix3d_amd/multiscale.py) ------------------------
 * MS-SSIM (Wang, Simoncelli, Bovik 2003) between two clips over a pyramid made on the device, in the integers of p3d_video.h's SSIM.  Why
 * here: as for the mesh decimation above — the video header's prototype list and the callers of its library are pinned by tests.
 *
 * A CLIP is uint8 [frames][h][w][bpp], 1 <= bpp <= 4, as in "frame resampling" below: pixels contiguous, any row and frame pitch, read in place.
 *
 * PYRAMID.  Level 0 is the clip.  Level k + 1 is floor(h / 2) x floor(w / 2); its sample (y, x, c) is
 *     (s[2y][2x][c] + s[2y][2x + 1][c] + s[2y + 1][2x][c] + s[2y + 1][2x + 1][c] + 2) >> 2
 * of level k: every channel on its own, one rounding, an odd last row or column dropped.  (NOT the 'box' filter of the resampling below, which
 * rounds once per pass.)
 *
 * PER LEVEL, for clips a (x) and b (y) of one size: the 11 x 11 window P3D_VIDEO_SSIM_WINDOW, the exact moments A, B, Pxx, Pyy, Pxy and the four
 * int64 factors n1, n2, d1, d2 of p3d_video_ssim (p3d_video.h states them; the constants are that header's), every window that lies inside the
 * picture, every channel on its own.  In fp64, every operator rounded once and none contracted:
 *     q  = ((double)n1 * (double)n2) / ((double)d1 * (double)d2)          (p3d_video_ssim's value)
 *     cs = (double)n2 / (double)d2                                        (contrast x structure; may be negative)
 * and the window contributes llrint(q 2^32) and llrint(cs 2^32) (round half to even).
 *
 * SUMS: int64 [3] per frame and channel = (sum of the q contributions, sum of the cs contributions, the number of windows).  The entry point ADDS
 * to them: integer sums, so neither the order of the work-groups nor that of the calls shows, and no call synchronises.
 *
 * ms_ssim = prod_{k < L - 1} max(cs_k, 0)^(w_k) * max(q_(L-1), 0)^(w_(L-1)) of the per-level means is fp64 work of the host (multiscale.py).   */
#define P3D_MSSSIM_MAX_LEVELS 5
#define P3D_MSSSIM_TILE_W 32              /* the work-group tile of p3d_frame_msssim_level, in PIXELS (tests straddle it); both are even, so */
#define P3D_MSSSIM_TILE_H 16              /* that no 2 x 2 block of the next level straddles two work-groups */

/* One clip to its next level: dst is [frames][h / 2][w / 2][bpp] with pitches of its own, apart from src.  A lane owns 4 consecutive output bytes
 * (12 at bpp 3: four pixels), which come from 8 (24) consecutive source bytes of two rows: dword loads and ONE dword store (three) where the two
 * source rows and the output row start on a dword, single bytes everywhere else and at a row's tail.  frames (h / 2) (w / 2) == 0 is a success
 * that launches nothing.  One launch.                                                                                                     */
int p3d_frame_halve(const uint8_t* src, int64_t src_frame_pitch, int64_t src_row_pitch, int32_t frames, int32_t h, int32_t w, int32_t bpp,
                    uint8_t* dst, int64_t dst_frame_pitch, int64_t dst_row_pitch, p3d_stream_t stream);

/* One level of a pair of clips: adds the level's three sums of frame f and channel c to sums[(f * bpp + c) * sums_pitch .. + 3) (sums_pitch in
 * int64 elements, >= 3: the caller's [frames][bpp][levels][3] has sums_pitch = 3 levels and passes the level's own address) and, with next_a
 * and next_b non-null (both or neither), writes the NEXT level of both clips, contiguous uint8 [frames][h / 2][w / 2][bpp] each, from the
 * samples it has staged.  h >= 11 and w >= 11: a level without a window is an error, never skipped.
 *
 * A work-group owns the P3D_MSSSIM_TILE_W x P3D_MSSSIM_TILE_H PIXELS at an even origin of one frame, all channels: the windows whose first
 * sample lies in the tile (their 42 x 26 samples go to LDS once, dwords where the addresses allow, no load past the frame) and the 16 x 8
 * samples of the next level under the tile.  The grid covers pixel tiles, ceil(w / 32) x ceil(h / 16) a frame: a work-group at the right or
 * bottom edge that owns no window still writes its share of the next level.  Per channel the moments run as in p3d_video_ssim (a horizontal
 * pass into LDS, a vertical pass a lane a window), the contributions meet in a wave reduction and the work-group issues ONE atomic per slot.
 * Every store is checked against the next level's sizes.  frames h w == 0 is a success that launches nothing; null a, b or sums (with
 * anything to do) returns P3D_ERR_ARGUMENT before any device call.  One launch.                                                          */
int p3d_frame_msssim_level(const uint8_t* a, int64_t a_frame_pitch, int64_t a_row_pitch, const uint8_t* b, int64_t b_frame_pitch,
                           int64_t b_row_pitch, int32_t frames, int32_t h, int32_t w, int32_t bpp, int64_t* sums, int64_t sums_pitch,
                           uint8_t* next_a, uint8_t* next_b, p3d_stream_t stream);

/* ---- frame resampling (csrc/sketch/frame_resample.hip; pix2pix3d_amd/resample.py) -------------------------------------
 * Pillow's Image.resize on 8-bit clips, bit for bit: for 8-bit samples it is integer arithmetic on fixed-point coefficient tables.  The tables
 * are made on the host (resample.py, Python floats); the three entry points below are the passes.  Why here: as for the mesh decimation above.
 *
 * A CLIP is uint8 [frames][h][w][bpp], 1 <= bpp <= 4: pixels contiguous, rows `*_row_pitch` bytes apart (>= w bpp), frames `*_frame_pitch` bytes
 * apart (>= 0; for a destination of more than one frame, at least the bytes of a frame).  1 <= h, w and every output size <= P3D_RESAMPLE_MAX_SIZE;
 * frames >= 0, and frames == 0 is a success that launches nothing.  All offsets are 64-bit.  Results are written out of place: the bytes the
 * destination spans must not meet the source's.  The channels of a pixel are resampled independently (PIL's L, RGB, RGBX; its LA / RGBA path
 * premultiplies alpha and is not this).
 *
 * Coefficients of one axis of in_size pixels resampled to out_size from the source interval [in0, in1) (default [0, in_size)).  Every float step
 * is IEEE double with one rounding per operator, in exactly this order.  A filter is a function f and a support S:
 *     box       f(x) = 1 if -0.5 < x <= 0.5, else 0                                                                        S = 0.5
 *     bilinear  f(x) = 1 - |x| if |x| < 1, else 0                                                                          S = 1
 *     hamming   f(x) = 1 if x == 0; 0 if |x| >= 1; otherwise with t = pi |x|: sin(t) / t * (0.54 + 0.46 cos(t))            S = 1
 *     bicubic   a = -0.5; |x| < 1: ((a + 2) |x| - (a + 3)) |x| |x| + 1;  |x| < 2: (((|x| - 5) |x| + 8) |x| - 4) a;  else 0  S = 2
 *     lanczos   sinc(x) sinc(x / 3) for -3 <= x < 3, else 0; sinc(0) = 1, otherwise with t = pi x: sin(t) / t              S = 3
 *   1. scale = (in1 - in0) / out_size, fs = max(scale, 1.0), support = S fs, ksize = int(ceil(support)) * 2 + 1.
 *   2. For the output xx: center = in0 + (xx + 0.5) scale.
 *   3. xmin = max(int(center - support + 0.5), 0).
 *   4. count = min(int(center + support + 0.5), in_size) - xmin.
 *   5. w[i] = f((i + xmin - center + 0.5) (1.0 / fs)) for i < count.
 *   6. ww = the sum of w[i] accumulated from 0.0 in index order; if ww != 0, w[i] = w[i] / ww.
 *   7. k[i] = int(-0.5 + w[i] 2^22) if w[i] < 0, else int(0.5 + w[i] 2^22); int truncates toward zero.
 *   8. Entries beyond count are 0.
 * The tables: bounds int32 [out_size][2] = (xmin, count) and weights int32 [out_size][ksize], with 255 sum |k| + 2^21 < 2^31 for every output
 * (resample.py checks it), so that the int32 accumulators never wrap.
 *
 * ONE PASS.  Each byte is out = min(max((2^21 + sum_i k[i] src[xmin + i]) >> 22, 0), 255): an arithmetic shift on int32, the sum per byte lane.
 * TWO AXES: the horizontal pass first, into a uint8 intermediate, then the vertical pass on it; the rounding to uint8 between the passes is part
 * of the definition.  The caller hands the horizontal pass only the source rows the vertical pass reads (a view: any row pitch will do).
 *
 * NEAREST: index tables int32 [ow] and [oh], made on the host by ACCUMULATION: s = in_size / out_size; xo = s 0.5; for each output
 * idx = min(int(xo), in_size - 1), then xo += s.  (The closed form int((x + 0.5) in_size / out_size) differs from it at some sizes.)
 *
 * Every kernel clamps what it reads from a table into the axis before use: xmin to [0, in_size], count to [0, min(ksize, in_size - xmin)], a
 * nearest index to [0, in_size - 1].  No load leaves a source row and no store leaves the output, whatever the tables hold.
 * Null pointers, sizes out of range, bpp outside 1 .. 4, ksize < 1 and pitches below the rows return P3D_ERR_ARGUMENT before any launch.      */
#define P3D_RESAMPLE_MAX_SIZE 32768       /* every side of a source or a result */
#define P3D_RESAMPLE_TILE_W 64            /* the work-group tile of the passes (tests straddle it): output pixels of the horizontal pass and of the */
#define P3D_RESAMPLE_TILE_H 16            /* gather, DWORDS of a row (4 P3D_RESAMPLE_TILE_W bytes) of the vertical pass; rows of all three */
#define P3D_RESAMPLE_LDS_ROW_BYTES 1024   /* the horizontal pass stages a tile's source span in LDS while it is at most this long a row ... */
#define P3D_RESAMPLE_LDS_TAPS 64          /* ... and ksize is at most this; a longer span or tap list is read from global memory directly */

/* The horizontal pass: dst[f][y][xx][c] from src[f][y][xmin(xx) + i][c]; dst is [frames][h][ow][bpp].  A work-group owns P3D_RESAMPLE_TILE_W output
 * pixels of P3D_RESAMPLE_TILE_H rows: it reads the bounds and the weights of its columns once (into LDS) and stages the source span those outputs
 * read, [the smallest xmin, the largest xmin + count) of every row of the tile, into LDS once — unless the span is longer than
 * P3D_RESAMPLE_LDS_ROW_BYTES or ksize exceeds P3D_RESAMPLE_LDS_TAPS (a 512 -> 1 Lanczos has 3073 taps), when every tap is read from global
 * memory.  One launch.                                                                                                                  */
int p3d_frame_resample_rows(const uint8_t* src, int64_t src_frame_pitch, int64_t src_row_pitch, int32_t frames, int32_t h, int32_t w, int32_t bpp,
                            uint8_t* dst, int64_t dst_frame_pitch, int64_t dst_row_pitch, int32_t ow, const int32_t* bounds, const int32_t* weights,
                            int32_t ksize, p3d_stream_t stream);

/* The vertical pass, channel-agnostic: a row is w bpp bytes and output byte j of row yy is the weighted sum of byte j over count(yy) source rows;
 * dst is [frames][oh][w][bpp].  A lane owns four consecutive bytes: a dword load where the source row's address allows and a dword store where
 * the output row's does, single bytes everywhere else (rows that start at an odd byte, the row's tail).  A wave owns one output row at a time,
 * so its bounds and weights are wave-uniform.  One launch.                                                                              */
int p3d_frame_resample_columns(const uint8_t* src, int64_t src_frame_pitch, int64_t src_row_pitch, int32_t frames, int32_t h, int32_t w, int32_t bpp,
                               uint8_t* dst, int64_t dst_frame_pitch, int64_t dst_row_pitch, int32_t oh, const int32_t* bounds,
                               const int32_t* weights, int32_t ksize, p3d_stream_t stream);

/* The gather: dst[f][yy][xx] = src[f][y_index[yy]][x_index[xx]], all bpp bytes; dst is [frames][oh][ow][bpp], x_index int32 [ow], y_index int32
 * [oh].  One launch.                                                                                                                    */
int p3d_frame_resample_nearest(const uint8_t* src, int64_t src_frame_pitch, int64_t src_row_pitch, int32_t frames, int32_t h, int32_t w, int32_t bpp,
                               uint8_t* dst, int64_t dst_frame_pitch, int64_t dst_row_pitch, int32_t oh, int32_t ow, const int32_t* x_index,
                               const int32_t* y_index, p3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
