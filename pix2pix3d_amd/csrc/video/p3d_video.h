/* libp3d_video.so — palette, dither and index frames for the GIF writer (pix2pix3d_amd/video.py) and, at the end, baseline JPEG
 * frames for the Motion-JPEG writer (section 2.1u).  A library of its
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

/* ---- baseline JPEG frames for the MJPEG writer (video_jpeg.hip) ------------------------------------------------------
 * Frames as above.  subsampling 0 is 4:4:4: the minimum coded unit (MCU) covers 8 x 8 pixels and holds 3 blocks, Y Cb Cr; subsampling 1 is 4:2:0:
 * the MCU covers 16 x 16 pixels and holds 6 blocks, Y00 Y01 Y10 Y11 Cb Cr (Yyx: the 8 x 8 quarter at row y, column x of the MCU).
 * mcus_x = ceil(w / mcu), mcus_y = ceil(h / mcu), n_mcu = mcus_x mcus_y in raster order; a clip with n_frames h w = 0 has no MCU and launches nothing.
 * Everything is integer arithmetic and a pure function of the inputs; the formulations of pix2pix3d_amd/video.py produce the same bytes.             */
#define P3D_VIDEO_JPEG_RESTART 8        /* MCUs of a restart interval: its 48 blocks are the lanes of ONE wave, their worst case 9948 bytes of LDS */
#define P3D_VIDEO_JPEG_BLOCK_BITS 1658  /* the longest coded block: 9 + 11 bits of DC, 63 coefficients of 16 + 10 bits */
/* T[u][x] = round(8192 a(u) cos((2 x + 1) u pi / 16)), a(0) = sqrt(1 / 8), a(u) = 1 / 2 otherwise: the rows of the integer DCT. */
#define P3D_VIDEO_JPEG_DCT_ROW0 2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896
#define P3D_VIDEO_JPEG_DCT_ROW1 4017, 3406, 2276, 799, -799, -2276, -3406, -4017
#define P3D_VIDEO_JPEG_DCT_ROW2 3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784
#define P3D_VIDEO_JPEG_DCT_ROW3 3406, -799, -4017, -2276, 2276, 4017, 799, -3406
#define P3D_VIDEO_JPEG_DCT_ROW4 2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896
#define P3D_VIDEO_JPEG_DCT_ROW5 2276, -4017, 799, 3406, -3406, -799, 4017, -2276
#define P3D_VIDEO_JPEG_DCT_ROW6 1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567
#define P3D_VIDEO_JPEG_DCT_ROW7 799, -2276, 3406, -4017, 4017, -3406, 2276, -799

/* coefficients int16 [n_frames][n_mcu][blocks of an MCU][64], every block in zigzag order.  luma_q, chroma_q uint8 [64], zigzag order, every entry >= 1
 * (a 0 counts as 1).  Per pixel, full-range JFIF in 16-bit fixed point (>> is an arithmetic shift throughout):
 *     Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *     Cb = clamp((-11059 R - 21709 G + 32768 B + 32768 + (128 << 16)) >> 16, 0, 255)
 *     Cr = clamp((32768 R - 27439 G - 5329 B + 32768 + (128 << 16)) >> 16, 0, 255)
 * The planes are padded to the MCU multiple by replicating the last row and column.  At 4:2:0 a chroma sample is (a + b + c + d + 2) >> 2 of a
 * 2 x 2 of the padded plane.  With s = sample - 128, the row pass is r[y][u] = (sum_x T[u][x] s[y][x] + 128) >> 8, the column pass
 * c8[v][u] = (sum_y T[v][y] r[y][u] + 16384) >> 15 — 8 x the orthonormal DCT; |r| <= 11584 and the column sum stays below 2^29 in int32.  The
 * coefficient is sign(c8) ((|c8| + 4 Q) / (8 Q)), an integer division, Q the table entry of its zigzag position.  ONE launch: a wave per block.  */
int p3d_video_jpeg_blocks(const uint8_t* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n_frames, int32_t h, int32_t w,
                          int32_t subsampling, const uint8_t* luma_q, const uint8_t* chroma_q, int16_t* coefficients, p3d_stream_t stream);

/* The entropy-coded scan of coefficients as p3d_video_jpeg_blocks lays them out, for a picture of h x w pixels.  A frame is cut into
 * n_intervals = ceil(n_mcu / P3D_VIDEO_JPEG_RESTART) restart intervals, the last one possibly shorter.  Every interval starts byte-aligned with the
 * DC predictors 0, is coded on its own, padded with 1-bits to a whole byte, byte-stuffed (a 0x00 after every 0xFF) and, unless it is the last of its
 * frame, followed by the marker 0xFF, 0xD0 + (interval index & 7).  Per block: the DC value (clamped to -1024 .. 1023) minus that of the previous block
 * of the same component in the interval (0 for the first), as the code of its size category and `size` extra bits; then for every non-zero AC value
 * (clamped to -1023 .. 1023) the code of ZRL (0xF0) once per 16 zeros before it, the code of (run & 15) << 4 | size and `size` extra bits; then the
 * code of EOB (0x00) unless coefficient 63 is non-zero.  The extra bits of v are v if v > 0 and v + 2^size - 1 otherwise.  huffman uint32 [4][256]
 * holds, per table (DC luma, DC chroma, AC luma, AC chroma: the chroma tables serve Cb and Cr) and symbol, length << 16 | code (length 1 .. 16).
 * data == NULL: lengths int32 [n_frames][n_intervals] receives the byte length of every interval, marker included.  data != NULL: every interval is
 * written at data + offsets[frame n_intervals + interval], offsets int64 [n_frames][n_intervals] being the exclusive prefix sum of those lengths (plus
 * whatever the caller leaves between frames); a byte at or past data_bytes is not written.  ONE launch either way: a wave per interval, a lane per
 * block; the bits are ORed into LDS words and leave the work-group as plain byte stores.                                                           */
int p3d_video_jpeg_scan(const int16_t* coefficients, int32_t n_frames, int32_t h, int32_t w, int32_t subsampling, const uint32_t* huffman,
                        int32_t* lengths, const int64_t* offsets, uint8_t* data, int64_t data_bytes, p3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
