/* libp3d_regions.so, continued: the cross-view consistency kernels (csrc/regions/view_reproject.hip; pix2pix3d_amd/reproject.py; DESIGN.md section
 * 2.1t).  Included at the end of p3d_regions.h, whose conventions hold: device pointers unless said otherwise, argument errors return
 * P3D_ERR_ARGUMENT before any launch, counters ACCUMULATE with 64-bit integer atomics into int64 memory the caller zeroed.  A header of its own
 * because pix2pix3d_amd/regions.py binds exactly what p3d_regions.h itself declares; reproject.py binds these three onto the same library.       */
#ifndef P3D_VIEW_REPROJECT_H
#define P3D_VIEW_REPROJECT_H
#include <stdint.h>
#include "../../../include/p3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* A forward warp between cameras: the pixels of one view, lifted to world points, are projected into another camera, the nearest point per
 * target pixel is kept (p3d_view_splat), labels and colours are carried across and the depths compared (p3d_view_resolve), and the carried
 * colours are compared with what the target view shows (p3d_view_difference_histogram).
 *
 * Sizes: a source view is h x w and a target view H x W pixels, each 1 .. P3D_PAINT_MAX_SIZE a side, and they may differ;
 * 0 <= frames <= 65536; frames == 0 is a success that launches nothing.  Counters ACCUMULATE.
 *
 * Cameras: float32 [frames][25], a camera label (views.camera_labels): the row-major 4 x 4 cam2world m (m03 = cameras[3], ...) followed by
 * the row-major normalised 3 x 3 intrinsics k (k0 = cameras[16], ...).  cam2world is taken to be a rigid motion: world -> camera is the
 * transposed rotation after the translation is taken off, no inverse is computed (the convention of mesh_project_kernel, csrc/mesh_raster.hip).
 *
 * Arithmetic: fp64 from the float32 operands, every operator rounded once (no contraction), in exactly this order.  The projection of a
 * world point P under the camera (m, k) into a W x H image:
 *     q  = P - (m03, m13, m23)
 *     xc = m00 qx;  xc = xc + m10 qy;  xc = xc + m20 qz        yc: column 1 (m01, m11, m21)        zc: column 2 (m02, m12, m22)
 *     a  = k0 xc;   a = a + k1 yc;     u = a / zc + k2         v = (k4 yc) / zc + k5
 *     sx = floor(u W),  sy = floor(v H),  zkey = floor(zc 65536)
 * The point is DROPPED when a component of P is not finite, or not zc > 0, or not zc 65536 < 2^31; a SPLAT point also when its valid byte is
 * 0 or not -4 <= sx < W + 4 or not -4 <= sy < H + 4 (tested on the doubles, before any conversion to an integer).  The torch formulation
 * of pix2pix3d_amd/reproject.py, fp64 element-wise ops in this order on CPU tensors, is the definition; the device bytes equal it.
 *
 * P3D_VIEW_EMPTY = INT64_MAX (0x7fffffffffffffff): a z-buffer cell nothing landed on.
 * Status of a target pixel: 0 hole, 1 consistent, 2 behind, 3 in front, 4 no target depth.
 *
 * Splat.  points float32 [frames or 1][h * w][3], point i = y * w + x, frames `points_frame_pitch` FLOATS apart (0: ONE source view seen by
 * every camera; else >= 3 h w).  valid: null or uint8 [frames or 1][h][w] with a row pitch (>= w) and a frame pitch (0: one map for every
 * frame; else >= (h - 1) * row pitch + w) in bytes.  radius 0, 1 or 2.  zbuf int64 [frames][H][W], contiguous, 8-byte aligned, which the
 * caller filled with P3D_VIEW_EMPTY (or with the keys of earlier splats).  For every point that is not dropped, key = zkey * 2^32 + i and
 *     zbuf[f][ty][tx] = min(zbuf[f][ty][tx], key)       for every in-image (tx, ty) with |tx - sx| <= radius and |ty - sy| <= radius
 * (a signed 64-bit atomic minimum: the smallest (zkey, i) wins whatever the order of arrival).  One launch.                              */
int p3d_view_splat(const float* points, int64_t points_frame_pitch, const uint8_t* valid, int64_t valid_row_pitch, int64_t valid_frame_pitch,
                   const float* cameras, int32_t frames, int32_t h, int32_t w, int32_t radius, int64_t* zbuf, int32_t H, int32_t W,
                   p3d_stream_t stream);

/* Resolve.  zbuf as p3d_view_splat left it.  src uint8 [frames or 1][h][w][channels], 1 <= channels <= 4 interleaved, rows `src_row_pitch`
 * (>= w * channels) and frames `src_frame_pitch` bytes apart (0: one source for every frame; else >= (h - 1) * row pitch + w * channels);
 * dst uint8 [frames][H][W][channels] with its own pitches (frame pitch not looked at for one frame), not overlapping src; fill (HOST memory,
 * read during the call): `channels` bytes.  index: null or int32 [frames][H][W], contiguous; status uint8 [frames][H][W], contiguous;
 * counts: null or int64 [5].  Per target pixel p = ty * W + tx, with key = zbuf[f][p], i = key & 0xffffffff, zk = key >> 32 (arithmetic):
 *     i >= h * w (P3D_VIEW_EMPTY is such a key; src is never read outside):  dst[f][p][c] = fill[c], index = -1, status 0
 *     otherwise:  dst[f][p][c] = src[f or 0][i / w][i % w][c], index = i, and the status
 *         target_points null:  1
 *         target_points float32 [frames][H * W][3], contiguous (the world points of the target view's own pixels), cameras as above and
 *         0 <= tolerance <= 2^31 - 1 in key units; zt = the zkey of target_points[f][p] under camera f:
 *             4 if that point is dropped (see above: the sx / sy range is not looked at here)
 *             1 if |zk - zt| <= tolerance
 *             2 if zk > zt   (the target sees a surface in front of the carried one: a disocclusion, not an error)
 *             3 otherwise    (the source puts matter where the target sees through: an inconsistency).
 * counts[s] += the pixels of status s.  One launch.                                                                                      */
int p3d_view_resolve(const int64_t* zbuf, const uint8_t* src, int64_t src_row_pitch, int64_t src_frame_pitch, int32_t h, int32_t w,
                     int32_t channels, const uint8_t fill[4], uint8_t* dst, int64_t dst_row_pitch, int64_t dst_frame_pitch, int32_t* index,
                     uint8_t* status, const float* target_points, const float* cameras, int64_t tolerance, int64_t* counts, int32_t frames,
                     int32_t H, int32_t W, p3d_stream_t stream);

/* Histogram of absolute differences.  a, b uint8 [frames][H][W][channels], 1 <= channels <= 4, each with a row pitch (>= W * channels) and a
 * frame pitch in bytes; where: null or uint8 [frames][H][W] with its pitches; 0 <= match <= 255; hist int64 [256].
 *     hist[|a[f][p][c] - b[f][p][c]|] += 1     for every channel c of every pixel with where[f][p] == match (of every pixel: where null).
 * One launch.                                                                                                                            */
int p3d_view_difference_histogram(const uint8_t* a, int64_t a_row_pitch, int64_t a_frame_pitch, const uint8_t* b, int64_t b_row_pitch,
                                  int64_t b_frame_pitch, const uint8_t* where, int64_t where_row_pitch, int64_t where_frame_pitch,
                                  int32_t match, int32_t channels, int32_t frames, int32_t H, int32_t W, int64_t* hist, p3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
