/* libp3d_video.so — palette, dither and index frames for the GIF writer (pix2pix3d_amd/video.py).  A library of its
 * own, like libp3d_regions.so: the product ABI (include/p3d_hip.h, libp3d_hip.so) exports none of this.  It carries its own copy of the
 * library services (p3d_last_error, p3d_launch_count).  Nothing here has a counterpart in the reference, which writes videos with imageio.
 *
 * Frames are uint8 [n_frames][h][w][3]: the three bytes of a pixel and the pixels of a row are contiguous, rows are `row_pitch` bytes apart
 * (>= 3 w) and frames `frame_pitch` bytes apart, so a strided selection of frames and a window of a larger canvas are read in place.
 * n_frames, h, w >= 0 and n_frames * h * w < 2^31; an empty clip launches nothing but the zeroing of the result.
 * A GROUP shares one histogram and one palette: the whole clip (per_frame = 0, n_groups = 1) or one frame (per_frame = 1, n_groups =
 * n_frames).  Everything is integer arithmetic and a pure function of the inputs: the torch formulations of pix2pix3d_amd/video.py produce
 * the same bytes.  All pointers are device memory.  Argument errors return P3D_ERR_ARGUMENT before any launch.                              */
#ifndef P3D_VIDEO_H
#define P3D_VIDEO_H
#include <stdint.h>
#include "../../../include/p3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define P3D_VIDEO_BINS 32768            /* 5 bits a channel: bin = (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3) */
#define P3D_VIDEO_COLORS 256            /* rows of a palette, boxes of a median cut */
#define P3D_VIDEO_MAX_AMPLITUDE 64

/* counts int32 [n_groups][P3D_VIDEO_BINS]: the number of pixels of the group in every bin.  Two launches: the first zeroes counts, the second
 * counts a share of one frame per work-group in LDS and adds its non-zero bins to counts.                                                   */
int p3d_video_histogram(const uint8_t* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n_frames, int32_t h, int32_t w,
                        int32_t per_frame, int32_t* counts, p3d_stream_t stream);

/* box_of_bin uint8 [n_groups][P3D_VIDEO_BINS]: the box of every bin.  sums int64 [n_groups][P3D_VIDEO_COLORS][4]: per box the sums of r, g
 * and b over the 8-bit colours of the pixels whose bin maps to it, and their number.  Two launches, as the histogram.                       */
int p3d_video_box_sums(const uint8_t* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n_frames, int32_t h, int32_t w,
                       int32_t per_frame, const uint8_t* box_of_bin, int64_t* sums, p3d_stream_t stream);

/* palette uint8 [n_groups][P3D_VIDEO_COLORS][3]; n_colors int32 [n_groups], read on the device and clamped to 1 .. P3D_VIDEO_COLORS: the rows
 * of the palette that count.  indices uint8 [n_frames][h][w], rows `index_row_pitch` (>= w) and frames `index_frame_pitch` bytes apart; it must
 * not overlap the frames.  For the pixel (x, y), with off = ((2 B8[y & 7][x & 7] - 63) * amplitude) >> 7 (an arithmetic shift) and
 * v' = min(max(v + off, 0), 255) per channel, the index is the k < n_colors with the smallest (r' - pr)^2 + (g' - pg)^2 + (b' - pb)^2, the
 * lowest such k.  B8 is the 8 x 8 Bayer matrix of the recursion M <- [[4M, 4M+2], [4M+3, 4M+1]] from [[0]]:
 * B8[y][x] = 16 q(y, x) + 4 q(y >> 1, x >> 1) + q(y >> 2, x >> 2) with q(y, x) = 2 ((x ^ y) & 1) + (y & 1).
 * 0 <= amplitude <= P3D_VIDEO_MAX_AMPLITUDE; 0 is no dither.  One launch.                                                                    */
int p3d_video_quantize(const uint8_t* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n_frames, int32_t h, int32_t w,
                       int32_t per_frame, const uint8_t* palette, const int32_t* n_colors, int32_t amplitude, uint8_t* indices,
                       int64_t index_frame_pitch, int64_t index_row_pitch, p3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
