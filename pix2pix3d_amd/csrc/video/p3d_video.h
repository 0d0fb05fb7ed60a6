/* libp3d_video.so — everything that works on uint8 clips.  For the writers: palette, dither and index frames of the GIFs (pix2pix3d_amd/video/gif.py; DESIGN.md
 * section 2.1q), baseline JPEG frames of the Motion-JPEG AVIs (section 2.1u), the zlib streams of PNG and APNG files (section 2.1v).  The way back from such
 * files: the JPEG entropy decoder (section 2.1y), inflate and un-filter (section 2.1z).  What a setting costs in the picture: error sums, SSIM and a decoder's
 * view of the JPEG coefficients (section 2.1x), MS-SSIM over a pyramid made on the device (section 2.1ac).  And the frames at another size: Pillow's resize
 * filters (section 2.1ab).  A library of its own, like libp3d_regions.so: the product ABI (include/p3d_hip.h, libp3d_hip.so) exports none of this.  It
 * carries its own copy of the library services (p3d_last_error, p3d_launch_count).  Nothing here has a counterpart in the reference, which writes videos
 * with imageio.
 *
 * A CLIP ("frames") is uint8 [n_frames][h][w][bpp]: the bpp bytes of a pixel and the pixels of a row are contiguous, rows are `row_pitch` bytes apart
 * (>= w bpp) and frames `frame_pitch` bytes apart (>= 0), so a strided selection of frames and a window of a larger canvas are read in place.  bpp is 3
 * for the GIF and JPEG stages, which take no such argument, and 1 .. 4 wherever an entry point takes it.  n_frames, h, w >= 0 and n_frames h w bpp < 2^31
 * (n_frames h w < 2^31 for the GIF and JPEG stages); an empty clip launches nothing but the zeroing of a result.  This is the one statement of the
 * contract: the sections below say only what they add to it.
 * A GROUP shares one histogram and one palette: the whole clip (per_frame = 0, n_groups = 1) or one frame (per_frame = 1, n_groups =
 * n_frames).  Everything is integer arithmetic and a pure function of the inputs: the torch formulations of pix2pix3d_amd/video/gif.py produce
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
 * Everything is integer arithmetic and a pure function of the inputs; the formulations of pix2pix3d_amd/video/jpeg.py produce the same bytes.        */
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

/* The way back from a file: the inverse of p3d_video_jpeg_scan for ANY baseline stream in restart intervals — ours, or libjpeg's with its own tables and its
 * own interval (video_jpeg_read.hip; the routine itself is jpeg_entropy.h, plain C++ that a host program runs as it stands).
 * data uint8 [data_bytes] holds the scans of all frames; ranges int64 [n_frames][n_intervals][2] the first byte of every interval and the byte after its
 * last, markers left out (clamped to 0 <= begin <= end <= data_bytes).  restart >= 1 MCUs an interval, n_intervals = ceil(n_mcu / restart), the last one
 * possibly shorter; a stream without restart markers is ONE interval of n_mcu MCUs (restart = n_mcu).  components 3: every MCU codes all its blocks;
 * components 1, with subsampling 0 only: a grey stream, whose MCU codes its Y block alone — the Cb and Cr blocks of the output stay zero.
 * TABLES.  tables uint32 [n_sets][4][P3D_VIDEO_JPEG_TABLE_WORDS], per set DC luma, DC chroma, AC luma, AC chroma, each made from a DHT's BITS / HUFFVAL
 * with the canonical codes of Annex C (code of the k-th value: they count up within a length, and a new length starts at twice the next code):
 *     [0 .. 255]    per 8-bit prefix: length << 16 | symbol of the code of length 1 .. 8 that the prefix starts with, 0 where there is none;
 *     [256 .. 271]  limit[l - 1], l = 1 .. 16: the last code of length l plus 1, 0 where no code has length l;
 *     [272 .. 287]  offset[l - 1], int32: the index in HUFFVAL of the first code of length l minus that code;
 *     [288 .. 351]  HUFFVAL, 256 bytes (zero-filled), byte i at bits 8 (i & 3) of word i >> 2.
 * A symbol: if the entry of the next 8 bits has a length 1 .. 8, that is it.  Otherwise, for l = 9 .. 16 in turn, with c the next l bits: the first l
 * with c < limit[l - 1] gives the symbol HUFFVAL[c + offset[l - 1]] if that index is 0 .. 255; no such l, or no such index: NO_CODE, and 16 bits count
 * as read.  table_of_frame int32 [n_frames]: the set of every frame (clamped to 0 .. n_sets - 1).
 * BITS.  An interval's bytes, most significant bit first; a 0x00 straight after a 0xFF inside the interval is dropped (any other byte after a 0xFF is
 * data, as is the 0xFF).  Past the interval's end the bits are zeros, and reading one sets EXHAUSTED.
 * BLOCKS, in the order p3d_video_jpeg_scan codes them, predictors 0 at the interval's start.  DC: a symbol `size` (> 11: SIZE), then `size` extra bits e:
 * the difference is e if e >= 2^(size - 1), else e - 2^size + 1; the value is the predictor of the component plus the difference, clamped to int16's
 * range, and becomes the predictor.  AC, from position z = 1 while z <= 63: a symbol run << 4 | size.  size = 0: run 0 ends the block, run 15 adds 16 to
 * z (z > 63 then: RUN — a value must follow), any other run: SIZE.  size > 10: SIZE.  Otherwise z += run (z > 63: RUN), the value of the extra bits goes
 * to position z, and z += 1.  After the last block, more than one whole data byte unread: LEFTOVER (up to 15 bits may pad an interval).
 * STATUS.  After every symbol and after every run of extra bits the status is looked at: with a bit set the interval ends there, what it has stored stays,
 * and the value in hand is not stored.  status int32 [n_frames][n_intervals] receives the bits; 0: the interval decoded cleanly.
 * coefficients int16 [n_frames][n_mcu][blocks of an MCU][64] as p3d_video_jpeg_blocks lays them out, so that p3d_video_jpeg_decode takes them as they are.
 * TWO launches: an asynchronous fill zeroes the coefficients (counted as one), then a lane per interval stores the non-zero values alone — a block's 128
 * bytes would otherwise be a scattered store per lane.  The frame's four tables sit in LDS.  No read leaves [begin, end), no store the frame's blocks,
 * and every loop is bounded, whatever the bytes and the tables hold.  n_frames h w = 0 launches nothing.                                                */
#define P3D_VIDEO_JPEG_LOOKUP_BITS 8
#define P3D_VIDEO_JPEG_TABLE_WORDS 352
#define P3D_VIDEO_JPEG_STATUS_NO_CODE 1     /* no code within 16 bits */
#define P3D_VIDEO_JPEG_STATUS_RUN 2         /* a run past position 63 */
#define P3D_VIDEO_JPEG_STATUS_SIZE 4        /* a DC size > 11, an AC size > 10, or an end-of-band symbol of progressive scans */
#define P3D_VIDEO_JPEG_STATUS_EXHAUSTED 8   /* bits read past the interval's end */
#define P3D_VIDEO_JPEG_STATUS_LEFTOVER 16   /* more than one whole byte unread */
int p3d_video_jpeg_unscan(const uint8_t* data, int64_t data_bytes, const int64_t* ranges, const uint32_t* tables, int32_t n_sets,
                          const int32_t* table_of_frame, int32_t n_frames, int32_t h, int32_t w, int32_t subsampling, int32_t components, int32_t restart,
                          int16_t* coefficients, int32_t* status, p3d_stream_t stream);

/* ---- lossless frames: the zlib streams of PNG and APNG files (video_png.hip) ------------------------------------------------
 * Pixels are bpp = 1 .. 4 bytes; the kernels know only bpp, the colour type is the file header's business ('L' 1, 'LA' and 16-bit grey 2, 'RGB' 3,
 * 'RGBA' 4, palette indices 1).  Frames uint8 [n_frames][h][w][bpp] with frame_pitch / row_pitch (>= w bpp) as above; n_frames h w bpp < 2^31 and
 * n_frames h (1 + w bpp) < 2^31; a clip with n_frames h w = 0 launches nothing.  Three stages, ONE launch each; integer arithmetic and a pure function
 * of the inputs throughout: the formulations of pix2pix3d_amd/video/png.py produce the same bytes.
 *
 * FILTER.  A row's filtered form is row_bytes = 1 + w bpp bytes: the filter type, then per byte x the residual (x - predictor) mod 256, with a the byte
 * bpp to the left (0 for the first pixel), b the byte above (0 in a frame's first row: every frame is filtered on its own) and c the byte above a.
 * Type 0 None: 0; 1 Sub: a; 2 Up: b; 3 Average: (a + b) >> 1; 4 Paeth: with p = a + b - c, pa = |p - a|, pb = |p - b|, pc = |p - c|: a if pa <= pb
 * and pa <= pc, else b if pb <= pc, else c.  filter 0 .. 4 forces a type; filter 5 (adaptive) takes, per row, the type with the smallest sum over
 * the row of |residual as int8| (r for r < 128, 256 - r otherwise), the lowest type on a tie.
 *
 * SEGMENTS.  segment_rows >= 1 consecutive filtered rows of a frame are a segment, the last of a frame possibly shorter: n_segments =
 * ceil(h / segment_rows) a frame.  A segment is coded on its own: no match and no bit crosses from one into the next.
 *
 * TOKENS of a segment.  Its bytes are cut into maximal runs of equal bytes.  A run of length n gives one literal; then, over the remaining m = n - 1
 * bytes, while m >= 3 a match of length min(m, 258) at distance 1; what remains, 1 or 2 bytes, as literals.  (By position: the byte k of a run,
 * k = 0 its first, carries a literal for k = 0; a match of 258 where k mod 258 = 0; and at the run's last byte, with r = k mod 258, a match of r for
 * r >= 3 and r literals for r = 1, 2.  No token needs more of the run than its own byte's k and whether the next byte differs.)  A match of length l
 * is the length symbol and extra bits of RFC 1951: 285 for 258; otherwise with v = l - 3, 257 + v for v < 8, else e = floor(log2 v) - 2 extra bits
 * of value v mod 2^e after the symbol 261 + 4 e + ((v >> e) & 3).  End of block (256) comes once per segment.
 *
 * CODES.  One literal/length code a FRAME, made on the host from the frame's symbol counts (256 counted once per segment): an optimal prefix code
 * under a limit of 15 bits, canonical as RFC 1951 section 3.2.2 assigns it.  The distance code is constant: symbols 0 and 1 with one bit each, so
 * a match costs one distance bit, a 0.  The dynamic block header — BTYPE = 10, HLIT, HDIST, HCLEN, the code-length code, the lengths — is made on
 * the host once a frame, as a bit string WITHOUT its BFINAL bit.
 *
 * BYTES of a segment, bits packed from the least significant bit of every byte on, as deflate packs them: BFINAL, the frame's header bits, the tokens
 * (a Huffman code from its most significant bit on, extra bits from their least), the code of 256.  Every segment but the frame's last has BFINAL = 0
 * and is followed by an empty stored block: the bits 000, zero bits up to the byte, then 00 00 FF FF — the next segment starts on a byte.  The last
 * has BFINAL = 1 and is padded with zero bits.  A frame's zlib stream is 78 01, its segments, and the big-endian Adler-32 of its filtered bytes.     */
#define P3D_VIDEO_PNG_SYMBOLS 286       /* literal/length symbols 0 .. 285 */
#define P3D_VIDEO_PNG_STATS 290         /* int32 a segment: [0 .. 285] symbol counts ([256] stays 0), [286] extra bits, [287] matches, [288] s1, [289] s2 */
#define P3D_VIDEO_PNG_HEADER_WORDS 144  /* uint32 a frame for the header bit string: 73 bits and 288 lengths of at most 7 + 7 bits fit 4105 */
#define P3D_VIDEO_PNG_ADAPTIVE 5        /* the filter argument that chooses per row */

/* filtered uint8 [n_frames][h][1 + w bpp], contiguous; it must not overlap the frames.  A wave per row: the five candidate sums by wave reductions, then
 * the type and the residuals as plain stores.                                                                                                          */
int p3d_video_png_filter(const uint8_t* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n_frames, int32_t h, int32_t w, int32_t bpp,
                         int32_t filter, uint8_t* filtered, p3d_stream_t stream);

/* stats int32 [n_frames][n_segments][P3D_VIDEO_PNG_STATS] of filtered rows of row_bytes (= 1 + w bpp) bytes: per segment the number of times every
 * literal/length symbol is coded (without 256), the sum of the matches' extra bits, the number of matches, and the Adler pair
 * s1 = sum b mod 65521, s2 = sum (L - i) b_i mod 65521 (i the 0-based index of byte b_i in the segment, L the segment's bytes).  n_frames h row_bytes
 * < 2^31; n_frames h = 0 or row_bytes <= 1 launches nothing.  A wave per segment, 64 bytes a step: a ballot of b[i] != b[i - 1] gives the run starts,
 * the length of the run left open is carried to the next step, the counts gather in LDS.                                                              */
int p3d_video_png_count(const uint8_t* filtered, int32_t n_frames, int32_t h, int32_t row_bytes, int32_t segment_rows, int32_t* stats,
                        p3d_stream_t stream);

/* tables uint32 [n_frames][P3D_VIDEO_PNG_SYMBOLS]: per frame and symbol, length << 16 | the code with its bits reversed (length 0 .. 15, more counts as
 * 15).  headers uint32 [n_frames][P3D_VIDEO_PNG_HEADER_WORDS]: the frame's header bit string, bit i at bit i & 31 of word i >> 5; header_bits int32
 * [n_frames] its length (clamped to 0 .. 32 P3D_VIDEO_PNG_HEADER_WORDS).  adler uint32 [n_frames]: the frame's Adler-32.  offsets int64
 * [n_frames][n_segments]: where in data every segment starts.  The segment's bytes, stored block included, go to data + offset; the first segment of a
 * frame also writes 78 01 to the two bytes before its own, the last the four bytes of adler after its own.  Nothing is written before data or at or
 * past data_bytes.  A wave per segment: the bits of 64 bytes are ORed into a window in LDS, whose whole words leave at once; a segment's output need
 * not fit LDS.                                                                                                                                         */
int p3d_video_png_emit(const uint8_t* filtered, int32_t n_frames, int32_t h, int32_t row_bytes, int32_t segment_rows, const uint32_t* tables,
                       const uint32_t* headers, const int32_t* header_bits, const uint32_t* adler, const int64_t* offsets, uint8_t* data,
                       int64_t data_bytes, p3d_stream_t stream);

/* ---- the way back from a lossless file: RFC 1951 inflate and the inverse of FILTER (video_png_read.hip, png_inflate.h) ----------
 * data uint8 [data_bytes]: raw deflate bytes — the zlib streams of all frames without their two header bytes and their four Adler bytes.  The bytes
 * need not come from us; the Python formulation of pix2pix3d_amd/video/png_read.py is the definition, the device result equals it.
 * PARTS.  parts int64 [n_parts][5]: in_begin, in_end, out_begin, out_end, final.  A part is a run of whole deflate blocks that begins on the first bit
 * of the byte in_begin; it is decoded on its own into out[out_begin, out_end).  in_begin / in_end are clamped to 0 .. data_bytes, out_begin / out_end
 * to 0 .. out_bytes, each end to no less than its begin.  A foreign stream is ONE part with final = 1; a stream whose segment boundaries are known is a
 * part a segment, the last alone with final = 1.  The out ranges of different parts must not overlap (where they do, any of their bytes may stand).
 * BITS.  A part's bytes, least significant bit first.  Past in_end the bits are zeros, and reading one sets EXHAUSTED.
 * BLOCKS.  BFINAL (1 bit), BTYPE (2 bits).  BTYPE 3: BLOCK_TYPE.  BFINAL = 1 in a part that is not final: BOUNDARY.
 *   Stored (0): the bits up to the next byte are skipped, then LEN and NLEN, 16 bits each; LEN != ~NLEN: STORED.  LEN bytes are copied; a byte at or
 *   past in_end: EXHAUSTED, else a byte for out_end or beyond: OVERFLOW.
 *   Fixed (1): the codes of RFC 1951 section 3.2.6 — literal/length lengths 8 (0 .. 143), 9 (.. 255), 7 (.. 279), 8 (.. 287), 32 distance codes of 5.
 *   Dynamic (2): HLIT + 257 (5 bits), HDIST + 1 (5), HCLEN + 4 (4); more than 286 literal/length or 30 distance codes: CODE_LENGTHS.  HCLEN lengths of
 *   3 bits for the code-length code in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, the rest 0.  Then HLIT + HDIST lengths under that
 *   code: 0 .. 15 a length; 16 the length before it 3 + (2 bits) times (nothing before it: CODE_LENGTHS); 17 zero 3 + (3 bits) times; 18 zero
 *   11 + (7 bits) times; a repeat past HLIT + HDIST: CODE_LENGTHS.  An over-subscribed code (sum of 2^-length over its used symbols above 1), of any
 *   of the three kinds: CODE_LENGTHS.  An incomplete code is accepted.
 * SYMBOLS.  Codes are canonical (RFC 1951 section 3.2.2), read from their most significant bit: the first length l = 1 .. 15 at which the bits so far
 * are a code of that length gives the symbol and l bits count as read; none: NO_CODE, and 15 bits count as read.  Literal/length 0 .. 255: the byte
 * (at or past out_end: OVERFLOW, and it is not written); 256 ends the block; 286 and 287: NO_CODE; else with k = symbol - 257 the length 3 + k
 * (k < 8), 258 (k = 28), else 3 + ((4 + (k & 3)) << e) + (e extra bits), e = (k - 4) >> 2.  Then a distance symbol d (30, 31: NO_CODE): 1 + d (d < 4),
 * else 1 + ((2 + (d & 1)) << e) + (e extra bits), e = (d >> 1) - 1.  A distance above the bytes the part has written: DISTANCE, and nothing is copied.
 * The match is copied byte by byte in order (an overlapping match repeats itself); a byte for out_end or beyond: OVERFLOW, the bytes before it stay.
 * THE END.  A final part ends after the block with BFINAL = 1: one or more whole bytes unread before in_end: LEFTOVER.  A part that is not final ends
 * after the first block that ends on the bit 8 in_end exactly.  Either kind that ends with fewer than out_end - out_begin bytes written: SHORT.
 * STATUS.  After every block header, every symbol and every run of extra bits the status is looked at: with a bit set the part ends there, what it wrote
 * stays, the rest of its range stays zero, and no other part is touched.  status int32 [n_parts] receives the bits; 0: the part decoded cleanly.
 * TWO launches: an asynchronous fill zeroes out (counted as one), then a lane per part, P3D_VIDEO_PNG_INFLATE_LANES lanes a work-group, the decode
 * tables of every lane in LDS.  No read leaves [in_begin, in_end), no store [out_begin, out_end), a match reads only inside [out_begin, out_end), and
 * every loop is bounded, whatever the bytes hold.  n_parts = 0 launches nothing.
 * WHY PARTS ARE SOUND.  If the parts of a stream tile its bytes and its output and every one reports 0, the bytes equal a serial decode: part 0 began
 * on a true block boundary and ended on its in_end after a whole block, so part 1 began on one, and so on; every count was exact; no match looked
 * outside its part.  A wrong list of parts shows as a status, never as a wrong picture.                                                                 */
#define P3D_VIDEO_PNG_INFLATE_LANES 32
#define P3D_VIDEO_PNG_STATUS_BLOCK_TYPE 1       /* BTYPE 3 */
#define P3D_VIDEO_PNG_STATUS_STORED 2           /* LEN != ~NLEN */
#define P3D_VIDEO_PNG_STATUS_CODE_LENGTHS 4     /* a dynamic header that describes no code */
#define P3D_VIDEO_PNG_STATUS_NO_CODE 8          /* no code within 15 bits, or a symbol that stands for nothing */
#define P3D_VIDEO_PNG_STATUS_DISTANCE 16        /* a match that reaches before the part's out_begin */
#define P3D_VIDEO_PNG_STATUS_OVERFLOW 32        /* a byte for out_end or beyond */
#define P3D_VIDEO_PNG_STATUS_EXHAUSTED 64       /* bits read past in_end */
#define P3D_VIDEO_PNG_STATUS_LEFTOVER 128       /* whole bytes unread after the final block */
#define P3D_VIDEO_PNG_STATUS_BOUNDARY 256       /* BFINAL = 1 in a part that is not final */
#define P3D_VIDEO_PNG_STATUS_SHORT 512          /* fewer bytes written than the part's range holds */
#define P3D_VIDEO_PNG_STATUS_FILTER 1024        /* a frame: a filter type above 4 (p3d_video_png_unfilter) */
#define P3D_VIDEO_PNG_STATUS_ADLER 2048         /* a frame: the Adler-32 of the inflated bytes is not the stream's (set by png_read.py) */
int p3d_video_png_inflate(const uint8_t* data, int64_t data_bytes, const int64_t* parts, int32_t n_parts, uint8_t* out, int64_t out_bytes,
                          int32_t* status, p3d_stream_t stream);

/* UNFILTER: the exact inverse of FILTER above.  filtered uint8 [n_frames][h][1 + w bpp], contiguous, as p3d_video_png_filter writes it, bpp = 1 .. 8
 * (6 and 8: 16-bit colour, which the file reader refuses but the rule does not).  Per byte x = (residual + predictor) mod 256, the predictor of the
 * row's type from the RECONSTRUCTED a (bpp bytes to the left, 0 for the first pixel), b (above, 0 in a frame's first row: every frame on its own) and
 * c (above a).  A type byte above 4 sets the frame's FILTER bit, and the row is taken as type 0.  frames uint8 [n_frames][h][w][bpp] with
 * frame_pitch / row_pitch (>= w bpp); bytes between rows stay untouched; it must not overlap filtered.  status int32 [n_frames]: 0 or FILTER.
 * n_frames h (1 + w bpp) < 2^31; n_frames h w = 0 launches nothing.  ONE launch: a wave a frame, a lane a row of a band of 64 rows, each lane one
 * pixel behind the lane above it.                                                                                                                       */
int p3d_video_png_unfilter(const uint8_t* filtered, int32_t n_frames, int32_t h, int32_t w, int32_t bpp, uint8_t* frames, int64_t frame_pitch,
                           int64_t row_pitch, int32_t* status, p3d_stream_t stream);

/* ---- frame quality: error sums, SSIM and what a decoder shows for JPEG coefficients (video_quality.hip, video_jpeg_decode.hip) ----
 * Two clips a and b, uint8 [n_frames][h][w][bpp], bpp = 1 .. 4, each with its own frame_pitch / row_pitch (>= w bpp) as above, are compared where they are.
 * n_frames, h, w >= 0 and n_frames h w bpp < 2^31.  The results ACCUMULATE into int64 counters that the caller zeroed: calls add up, in any order (integer
 * sums), and nothing waits for the host.  Integer arithmetic and a pure function of the inputs but for the three fp64 operations stated below: the
 * formulations of pix2pix3d_amd/quality.py produce the same bytes.
 *
 * ERROR SUMS.  With d = a - b per sample, sums int64 [n_frames][bpp][4] gains, per frame and channel: sum |d|, sum d^2, max |d| (a 64-bit atomic max) and
 * the number of samples with d != 0.  A clip with n_frames h w = 0 launches nothing.  ONE launch: registers, a wave reduction, LDS, then one atomic per
 * slot per work-group.                                                                                                                                     */
int p3d_video_error_sums(const uint8_t* a, int64_t a_frame_pitch, int64_t a_row_pitch, const uint8_t* b, int64_t b_frame_pitch, int64_t b_row_pitch,
                         int32_t n_frames, int32_t h, int32_t w, int32_t bpp, int64_t* sums, p3d_stream_t stream);

/* SSIM (Wang, Bovik, Sheikh, Simoncelli 2004): 11 x 11 Gaussian window of sigma 1.5, K1 = 0.01, K2 = 0.03, L = 255, the (h - 10) x (w - 10) windows that
 * lie wholly inside the picture, every channel on its own.  The 1-D window is g[i] = round(1024 exp(-(i - 5)^2 / 4.5) / sum_j exp(-(j - 5)^2 / 4.5)), which
 * sums to 1024; the 2-D weights are w[i][j] = g[i] g[j], their sum S = 2^20.  With x the samples of a and y those of b in a window, exact integers:
 *     A = sum w x, B = sum w y (< 2^28);   Pxx = sum w x^2, Pyy = sum w y^2, Pxy = sum w x y (< 2^36)
 * (the horizontal pass fits int32, the vertical one is int64 for the three products), and with C1 = round((0.01 255)^2 2^40), C2 = round((0.03 255)^2 2^40):
 *     n1 = 2 A B + C1              n2 = 2 (S Pxy - A B) + C2
 *     d1 = A^2 + B^2 + C1          d2 = S (Pxx + Pyy) - A^2 - B^2 + C2
 * four int64 below 2^59 in magnitude; d1 >= C1 > 0 and, by Cauchy-Schwarz (S Pxx >= A^2), d2 >= C2 > 0.  Each is converted to fp64 (round to nearest even),
 * q = (n1 n2) / (d1 d2) is three fp64 operations in that order, none contracted, and the window contributes the int64 round_half_even(q 2^32) (llrint).
 * sums int64 [n_frames][bpp][2] gains the sum of the contributions and the number of windows; map, if non-null, float32 [n_frames][h - 10][w - 10][bpp],
 * contiguous, receives (float) q.  h < 11 or w < 11 or n_frames = 0: no window, no launch.  ONE launch: a work-group per tile of
 * P3D_VIDEO_SSIM_TILE_W x P3D_VIDEO_SSIM_TILE_H windows of one frame.                                                                                     */
#define P3D_VIDEO_SSIM_WINDOW 1, 8, 37, 112, 218, 272, 218, 112, 37, 8, 1
#define P3D_VIDEO_SSIM_TAPS 11
#define P3D_VIDEO_SSIM_C1 7149574359613LL
#define P3D_VIDEO_SSIM_C2 64346169236521LL
#define P3D_VIDEO_SSIM_SHIFT 32         /* a window contributes round(q 2^32) */
#define P3D_VIDEO_SSIM_TILE_W 32
#define P3D_VIDEO_SSIM_TILE_H 16
int p3d_video_ssim(const uint8_t* a, int64_t a_frame_pitch, int64_t a_row_pitch, const uint8_t* b, int64_t b_frame_pitch, int64_t b_row_pitch,
                   int32_t n_frames, int32_t h, int32_t w, int32_t bpp, int64_t* sums, float* map, p3d_stream_t stream);

/* What a decoder shows for coefficients as p3d_video_jpeg_blocks lays them out (no entropy decoding: a quality setting is judged where the frames are).
 * DEQUANTISE: coefficient x table entry of its zigzag position (a 0 entry counts as 1), clamped to -32768 .. 32767.  INVERSE TRANSFORM with the table T of
 * the forward pass, on the block c[v][u] in natural order: the column pass m[y][u] = (sum_v T[v][y] c[v][u] + 512) >> 10, then the row pass
 * s[y][x] = (sum_u T[u][x] m[y][u] + 32768) >> 16 — 26 bits in all: T is 8192 x orthonormal, twice, and the quantiser's division by 8 Q has already taken
 * the forward pass's factor 8 out, so c is the orthonormal DCT itself.  sum_v |T[v][y]| = 21641, so the first sum stays below 21641 x 32768 + 512 < 2^30
 * in int32 and |m| <= 692513; the second, up to 21641 x 692513 > 2^31, is an int64 sum.  The sample is clamp(s + 128, 0, 255).  PLANES: Y of (mcus_y mcu) x (mcus_x mcu) samples, Cb and Cr the same (4:4:4) or half of it each way (4:2:0); scratch
 * holds them, uint8, frame after frame, Y then Cb then Cr: scratch_bytes >= n_frames x (the Y plane + the two chroma planes).  UPSAMPLING at 4:2:0, on the
 * chroma plane cropped to ceil(h / 2) x ceil(w / 2) with its edges replicated — the triangle filter: for the output row y, v[cx] = 3 near + far, near the
 * chroma row y >> 1 and far the row above it for even y, below it for odd y; for the output column x, with cx = x >> 1, (3 v[cx] + v[cx - 1] + 8) >> 4 for
 * even x and (3 v[cx] + v[cx + 1] + 7) >> 4 for odd x.  COLOUR, full-range JFIF in 16-bit fixed point (>> arithmetic), each clamped to 0 .. 255:
 *     R = Y + ((91881 (Cr - 128) + 32768) >> 16)          B = Y + ((116130 (Cb - 128) + 32768) >> 16)
 *     G = Y + ((-22554 (Cb - 128) - 46802 (Cr - 128) + 32768) >> 16)
 * frames uint8 [n_frames][h][w][3] with frame_pitch / row_pitch (>= 3 w) receives the h x w crop; bytes between rows stay untouched.  n_frames h w = 0
 * launches nothing.  TWO launches: a wave per block into the planes, then a thread per pixel.                                                             */
int p3d_video_jpeg_decode(const int16_t* coefficients, int32_t n_frames, int32_t h, int32_t w, int32_t subsampling, const uint8_t* luma_q,
                          const uint8_t* chroma_q, uint8_t* scratch, int64_t scratch_bytes, uint8_t* frames, int64_t frame_pitch, int64_t row_pitch,
                          p3d_stream_t stream);

/* ---- multi-scale frame quality (frame_multiscale.hip, ssim_window.h; pix2pix3d_amd/multiscale.py) ------------------------
 * MS-SSIM (Wang, Simoncelli, Bovik 2003) between two clips over a pyramid made on the device, in the integers of the SSIM above.
 *
 * PYRAMID.  Level 0 is the clip.  Level k + 1 is floor(h / 2) x floor(w / 2); its sample (y, x, c) is
 *     (s[2y][2x][c] + s[2y][2x + 1][c] + s[2y + 1][2x][c] + s[2y + 1][2x + 1][c] + 2) >> 2
 * of level k: every channel on its own, one rounding, an odd last row or column dropped.  (NOT the 'box' filter of the resampling below, which
 * rounds once per pass.)
 *
 * PER LEVEL, for clips a (x) and b (y) of one size: the 11 x 11 window P3D_VIDEO_SSIM_WINDOW, the exact moments A, B, Pxx, Pyy, Pxy and the four
 * int64 factors n1, n2, d1, d2 of p3d_video_ssim above, every window that lies inside the
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

/* ---- frame resampling (frame_resample.hip; pix2pix3d_amd/resample.py) -------------------------------------
 * Pillow's Image.resize on 8-bit clips, bit for bit: for 8-bit samples it is integer arithmetic on fixed-point coefficient tables.  The tables
 * are made on the host (resample.py, Python floats); the three entry points below are the passes.
 *
 * Source and destination are clips, each with its own pitches; a destination of more than one frame has a frame pitch of at least the bytes of a
 * frame.  1 <= h, w and every output size <= P3D_RESAMPLE_MAX_SIZE; frames == 0 is a success that launches nothing.  All offsets are 64-bit.
 * Results are written out of place: the bytes the destination spans must not meet the source's.  The channels of a pixel are resampled
 * independently (PIL's L, RGB, RGBX; its LA / RGBA path premultiplies alpha and is not this).
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
