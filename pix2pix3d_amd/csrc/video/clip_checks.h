// The host-side argument checks that the entry points on a pair of clips share (video_quality.hip, frame_multiscale.hip): p3d_video.h's clip contract for
// bpp = 1 .. 4.  Each returns P3D_OK or sets the library's error and returns P3D_ERR_ARGUMENT; nothing here touches the device.
#ifndef P3D_CLIP_CHECKS_H
#define P3D_CLIP_CHECKS_H
#include "../p3d_common.h"

namespace p3d {

// The sizes of one clip; *pixels = n_frames h w.
inline int check_clip_sizes(const char* what, int32_t n_frames, int32_t h, int32_t w, int32_t bpp, int64_t* pixels)
{
    P3D_REQUIRE(n_frames >= 0 && h >= 0 && w >= 0, "%s: n_frames, h and w must be >= 0 (got %d, %d, %d)", what, n_frames, h, w);
    P3D_REQUIRE(bpp >= 1 && bpp <= 4, "%s: bpp must be 1 .. 4 (got %d)", what, bpp);
    const int64_t hw = (int64_t)h * w;
    P3D_REQUIRE(hw < (1ll << 31) && hw * n_frames * bpp < (1ll << 31), "%s: %d x %d x %d pixels of %d bytes reach 2^31", what, n_frames, h, w, bpp);
    *pixels = hw * n_frames;
    return P3D_OK;
}

// Two clips of one size and the int64 counters they are measured into; with no pixel there is nothing to read and no pointer is looked at.
inline int check_pair(const char* what, const uint8_t* a, int64_t a_frame_pitch, int64_t a_row_pitch, const uint8_t* b, int64_t b_frame_pitch,
                      int64_t b_row_pitch, int32_t n_frames, int32_t h, int32_t w, int32_t bpp, const int64_t* sums, int64_t* pixels)
{
    if (int code = check_clip_sizes(what, n_frames, h, w, bpp, pixels)) return code;
    if (*pixels == 0) return P3D_OK;
    P3D_REQUIRE(a && b && sums, "%s: a, b and sums must be non-null", what);
    P3D_REQUIRE(((uintptr_t)sums & 7u) == 0, "%s: sums must be 8-byte aligned", what);
    P3D_REQUIRE(a_row_pitch >= (int64_t)w * bpp && b_row_pitch >= (int64_t)w * bpp && a_frame_pitch >= 0 && b_frame_pitch >= 0,
                "%s: a row pitch is shorter than the row, or a frame pitch negative", what);
    return P3D_OK;
}

} // namespace p3d
#endif
