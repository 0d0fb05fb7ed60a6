/* libp3d_regions.so — region tools on the uint8 label map of an edit session (pix2pix3d_amd/regions.py).  A library of
 * its own, like libp3d_probes.so: the product ABI (include/p3d_hip.h, libp3d_hip.so) exports none of this.  It carries its own copy of the
 * library services (p3d_last_error, p3d_launch_count).  Nothing here has a counterpart in the reference, whose demo edits with the mouse only.
 *
 * Every mask is uint8 [h][w], pixels contiguous, rows `*_row_pitch` bytes apart (>= w); 1 <= h, w <= P3D_PAINT_MAX_SIZE.  Every result is
 * written out of place and is a pure function of the inputs: the torch formulations of pix2pix3d_amd/regions.py produce the same bytes.
 * All pointers are device memory unless said otherwise.  Argument errors return P3D_ERR_ARGUMENT before any launch.                        */
#ifndef P3D_REGIONS_H
#define P3D_REGIONS_H
#include <stdint.h>
#include "../../../include/p3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Connected components of equal labels under the 4- or 8-neighbourhood (`connectivity`; anything else is an argument error).
 * ids int32 [h][w], contiguous: every pixel gets the smallest linear index y * w + x of its component.  Three launches (init, hook,
 * flatten): union-find in the protocol of csrc/mesh_ops.hip; ids is the parent array.                                                    */
int p3d_label_components(const uint8_t* mask, int64_t mask_row_pitch, int32_t* ids, int32_t h, int32_t w, int32_t connectivity,
                         p3d_stream_t stream);

/* Nearest site.  `sites` (HOST memory, read during the call): 256 bits, label l is a site label iff sites[l / 32] >> (l % 32) & 1.
 * nearest int32 [h][w], contiguous: the linear index of the site pixel with the smallest (d^2, index), d^2 the squared Euclidean pixel
 * distance; a site gets itself; -1 when there is no site or when radius >= 0 and d^2 > radius^2 (radius < 0: unbounded).
 * workspace int32 [h * w]: pass 1 leaves there, per pixel, the nearest site row within the pixel's own column (the upper one on a tie, -1
 * for none); pass 2 takes the minimum of ((x - x')^2 + (y - sy(x'))^2, sy(x') * w + x') over the columns x'.  Two launches.              */
int p3d_label_nearest(const uint8_t* mask, int64_t mask_row_pitch, const uint32_t sites[8], int32_t radius, int32_t* workspace,
                      int32_t* nearest, int32_t h, int32_t w, p3d_stream_t stream);

/* Inverse affine warp of a region.  `coef` (HOST memory, read during the call): six integers in 1 / 65536 pixel, the linear ones within
 * +-2^22 and the translations coef[2], coef[5] within +-2^40.  For the destination pixel (px, py):
 *     qx = (coef[0] px + coef[1] py + coef[2] + 32768) >> 16,   qy = (coef[3] px + coef[4] py + coef[5] + 32768) >> 16   (arithmetic shifts)
 *     dst[py][px] = q inside the image and region[qy][qx] != 0 ? mask[qy][qx] : under[py][px].
 * dst must not overlap the other three.  One launch.                                                                                     */
int p3d_label_warp(const uint8_t* mask, int64_t mask_row_pitch, const uint8_t* region, int64_t region_row_pitch, const uint8_t* under,
                   int64_t under_row_pitch, uint8_t* dst, int64_t dst_row_pitch, const int64_t coef[6], int32_t h, int32_t w,
                   p3d_stream_t stream);

/* ---- agreement metrics (csrc/regions/label_metrics.hip; pix2pix3d_amd/evaluate.py) ----------------------------
 * The three counters below ACCUMULATE (+=, 64-bit integer atomics: the sums do not depend on the order) into int64 device memory, 8-byte
 * aligned, that the caller zeroed: a loop over a dataset never touches the host.
 *
 * Confusion matrix.  truth, pred and the optional valid (null: every pixel is valid): uint8 [frames][h][w], rows `*_row_pitch` bytes apart
 * and frames `*_frame_pitch` bytes apart (>= (h - 1) * row pitch + w; not looked at for one frame); 0 <= frames <= 65536,
 * 1 <= n_labels <= 32.  counts int64 [n_labels * n_labels + 1]:
 *     counts[t * n_labels + p] += pixels with truth == t, pred == p, both < n_labels, and valid != 0
 *     counts[n_labels * n_labels] += pixels left out for any of those reasons.
 * frames == 0 is a success that launches nothing.  One launch.                                                                          */
int p3d_label_confusion(const uint8_t* truth, int64_t truth_row_pitch, int64_t truth_frame_pitch, const uint8_t* pred,
                        int64_t pred_row_pitch, int64_t pred_frame_pitch, const uint8_t* valid, int64_t valid_row_pitch,
                        int64_t valid_frame_pitch, int32_t frames, int32_t h, int32_t w, int32_t n_labels, int64_t* counts,
                        p3d_stream_t stream);

/* Boundary map.  out[p] = mask[p] if some in-image 4-neighbour of p has a different label, else 255.  (A pixel labelled 255 is therefore
 * never a boundary pixel itself, but it counts as different to its neighbours.)  p3d_label_nearest of the result with the site set {c} is
 * then "the nearest boundary pixel of class c", with the set 0 .. 254 the class-agnostic boundary.  The byte ranges of mask and out must not
 * overlap.  One launch.                                                                                                                 */
int p3d_label_boundary(const uint8_t* mask, int64_t mask_row_pitch, uint8_t* out, int64_t out_row_pitch, int32_t h, int32_t w,
                       p3d_stream_t stream);

/* Histogram of squared distances.  `sites` (HOST memory, read during the call): the 256-bit label set of p3d_label_nearest.  nearest int32
 * [h][w], contiguous, as p3d_label_nearest wrote it for the OTHER map; 1 <= bins <= 4096; hist int64 [bins + 2].  For every pixel p = (px, py)
 * whose `from` label is in the set, with q = nearest[p] = qy * w + qx and d2 = (px - qx)^2 + (py - qy)^2:
 *     q >= 0 and d2 <  bins:  hist[d2] += 1
 *     q >= 0 and d2 >= bins:  hist[bins] += 1
 *     q <  0:                 hist[bins + 1] += 1.
 * A q >= h * w is NOT checked on the device (it only yields a large d2): the pointer contract is the caller's.  One launch.               */
int p3d_label_distance_histogram(const uint8_t* from, int64_t from_row_pitch, const uint32_t sites[8], const int32_t* nearest, int32_t bins,
                                 int64_t* hist, int32_t h, int32_t w, p3d_stream_t stream);

#ifdef __cplusplus
}
#endif

/* The cross-view consistency kernels of the same library (csrc/regions/view_reproject.hip) are declared in a header of their own, which every
 * includer of this one sees: pix2pix3d_amd/regions.py binds the six prototypes above, pix2pix3d_amd/reproject.py the three of that header.  */
#include "p3d_view_reproject.h"
#endif
