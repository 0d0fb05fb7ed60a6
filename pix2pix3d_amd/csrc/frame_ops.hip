// Displayable frames on the device: p3d_frame_finish turns the float outputs of a chunk of views (image, label logits, depth) into
// uint8 frames in ONE launch — what the reference's scripts do per frame on the host after a synchronising copy
// (applications/generate_video.py:65-67, 81-82; generate_samples.py:116-120; training/utils.py:5-15).
//
// A thread owns up to four consecutive pixels of one row.  The groups of a row are laid out from the DESTINATION's alignment: group 0 is the
// (at most three pixel) head in front of the first 4-byte boundary of the row, group g >= 1 starts on a boundary — four 3-byte pixels are three
// whole dwords, four 1-byte pixels one — so every full group is stored as dwords and only a row's head and tail fall back to byte stores.
// Sources are read through element strides on one of three paths, chosen per job on the host:
//   planar        (x stride 1): per channel the four pixels are 16 contiguous bytes — one 16-byte load where the address allows, four dwords otherwise;
//   channels-last (c stride 1): per pixel four channels are 16 contiguous bytes — 16- / 8- / 4-byte loads by the alignment of pointer and strides;
//   strided       anything else, dword loads.
// All three feed the same arithmetic, so they give the same bytes.  Loads are issued a block (4 channels x 4 pixels) ahead of their use and never
// under a data-dependent branch (out-of-range channels / pixels re-read a valid neighbour and are ignored).
#include "p3d_common.h"

namespace {

using namespace p3d;

constexpr int kMaxJobs = P3D_FRAME_MAX_JOBS;
constexpr int kPlanar = 0, kChannelsLast = 1, kStrided = 2;

struct FrameJob {
    const float* src; int64_t sn, sc, sy, sx;
    uint8_t* dst; int64_t drow, dframe;             // dst / idx already point at the rectangle's origin
    uint8_t* idx; int64_t irow, iframe;
    const uint8_t* pal_dev;
    int mode, N, C, H, W, bpp, groups, path, vec;
    float lo, scale;
    unsigned pal[64];                               // by-value palette, one R | G << 8 | B << 16 dword per label
};
struct FrameArgs { FrameJob job[kMaxJobs]; int first_block[kMaxJobs + 1]; int njobs; };

// u8 = (uint8)clamp((x - lo) * s, 0, 255): two separately rounded fp32 operations (never one FMA), truncation toward zero, NaN -> 0
__device__ __forceinline__ unsigned scale_u8(float x, float lo, float s)
{
    const float t = __fmul_rn(__fsub_rn(x, lo), s);
    const float r = t > 0.f ? fminf(t, 255.f) : 0.f;        // (a NaN fails the comparison)
    return (unsigned)r;
}

// v[k][i] = channel c0 + k of pixel i of the thread's group.  Channels >= C are skipped (a launch-uniform test) or re-read a valid neighbour, pixels >= cnt
// read pixel cnt - 1: every address is valid and no load sits under a per-lane branch; the caller ignores what is out of range.
template <int PATH>
__device__ __forceinline__ void load_block(const FrameJob& q, const float* base, int c0, int cnt, float (&v)[4][4])
{
    const int C = q.C;
    if (PATH == kPlanar) {
        const bool vec_ok = cnt == 4 && q.vec == 4 && (((uintptr_t)base) & 15u) == 0;      // (vec == 4: every channel plane keeps the row's alignment)
        if (vec_ok) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (c0 + k < C) {
                    const float4 t = *(const float4*)(base + (int64_t)(c0 + k) * q.sc);
                    v[k][0] = t.x; v[k][1] = t.y; v[k][2] = t.z; v[k][3] = t.w;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (c0 + k < C) {
                    const float* p = base + (int64_t)(c0 + k) * q.sc;
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[k][i] = p[min(i, cnt - 1)];
                }
            }
        }
    } else if (PATH == kChannelsLast) {
        if (q.vec == 4 && c0 + 4 <= C) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 t = *(const float4*)(base + (int64_t)min(i, cnt - 1) * q.sx + c0);
                v[0][i] = t.x; v[1][i] = t.y; v[2][i] = t.z; v[3][i] = t.w;
            }
        } else if (q.vec >= 2 && c0 + 2 <= C) {                                            // (C even here, see the host: c0 + 2 may be the last pair)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float* p = base + (int64_t)min(i, cnt - 1) * q.sx;
                const float2 t0 = *(const float2*)(p + c0);
                const float2 t1 = *(const float2*)(p + min(c0 + 2, C - 2));
                v[0][i] = t0.x; v[1][i] = t0.y; v[2][i] = t1.x; v[3][i] = t1.y;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float* p = base + (int64_t)min(i, cnt - 1) * q.sx;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k][i] = p[min(c0 + k, C - 1)];
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (c0 + k < C) {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[k][i] = base[(int64_t)(c0 + k) * q.sc + (int64_t)min(i, cnt - 1) * q.sx];
            }
        }
    }
}

// cnt bytes-per-pixel groups at p: whole dwords when `packed` (the caller guarantees 4-byte alignment and cnt == 4), bytes otherwise
__device__ __forceinline__ void store_pixels(uint8_t* p, const unsigned (&b)[12], int nbytes, bool packed)
{
    if (packed) {
        unsigned* d = (unsigned*)p;
        d[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        if (nbytes == 12) {
            d[1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
            d[2] = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
        }
    } else {
#pragma unroll
        for (int t = 0; t < 12; ++t)
            if (t < nbytes) p[t] = (uint8_t)b[t];
    }
}

template <int PATH>
__device__ __forceinline__ void frame_job(const FrameJob& q, int64_t e)
{
    const int64_t total = (int64_t)q.N * q.H * q.groups;
    if (e >= total) return;
    const int g = (int)(e % q.groups);
    const int64_t row = e / q.groups;
    const int y = (int)(row % q.H), n = (int)(row / q.H);
    uint8_t* const drow = q.dst + (int64_t)n * q.dframe + (int64_t)y * q.drow;
    const int mis = (int)(((uintptr_t)drow) & 3u);
    const int head = q.bpp == 3 ? mis : ((4 - mis) & 3);            // pixels in front of the row's first 4-byte boundary that starts a pixel
    const int x0 = g == 0 ? 0 : head + 4 * (g - 1);
    const int x1 = g == 0 ? min(head, q.W) : min(q.W, x0 + 4);
    const int cnt = x1 - x0;
    if (cnt <= 0) return;
    const bool packed = g > 0 && cnt == 4;
    const float* const base = q.src + (int64_t)n * q.sn + (int64_t)y * q.sy + (int64_t)x0 * q.sx;
    uint8_t* const dp = drow + (int64_t)x0 * q.bpp;

    float cur[4][4] = {};
    load_block<PATH>(q, base, 0, cnt, cur);
    unsigned b[12];
#pragma unroll
    for (int t = 0; t < 12; ++t) b[t] = 0;
    if (q.mode == P3D_FRAME_SCALE) {
        if (q.bpp == 3) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) b[i * 3 + k] = scale_u8(cur[k][i], q.lo, q.scale);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) b[i] = scale_u8(cur[0][i], q.lo, q.scale);
        }
        store_pixels(dp, b, cnt * q.bpp, packed);
        return;
    }
    // LABEL: argmax over the channels by torch.argmax's CPU rules — the first maximal channel wins, a NaN is the maximum and the first NaN wins
    float best[4];
    unsigned bk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { best[i] = cur[0][i]; bk[i] = 0; }
    const int C = q.C;
    for (int c0 = 0; c0 < C; c0 += 4) {
        float nxt[4][4] = {};
        if (c0 + 4 < C) load_block<PATH>(q, base, c0 + 4, cnt, nxt);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (c0 + k < C && c0 + k > 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = cur[k][i];
                    const bool take = (v > best[i]) || (v != v && best[i] == best[i]);
                    best[i] = take ? v : best[i];
                    bk[i] = take ? (unsigned)(c0 + k) : bk[i];
                }
            }
        }
        if (c0 + 4 < C) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i) cur[k][i] = nxt[k][i];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned rgb;
        if (q.pal_dev) {
            const uint8_t* pe = q.pal_dev + bk[i] * 3;
            rgb = (unsigned)pe[0] | ((unsigned)pe[1] << 8) | ((unsigned)pe[2] << 16);
        } else {
            rgb = q.pal[bk[i]];
        }
        b[i * 3 + 0] = rgb & 255u; b[i * 3 + 1] = (rgb >> 8) & 255u; b[i * 3 + 2] = (rgb >> 16) & 255u;
    }
    store_pixels(dp, b, cnt * 3, packed);
    if (q.idx) {
        uint8_t* const ip = q.idx + (int64_t)n * q.iframe + (int64_t)y * q.irow + x0;
        unsigned kb[12];
#pragma unroll
        for (int t = 0; t < 12; ++t) kb[t] = t < 4 ? bk[t & 3] : 0u;
        store_pixels(ip, kb, cnt, cnt == 4 && (((uintptr_t)ip) & 3u) == 0);
    }
}

__global__ void __launch_bounds__(256) frame_finish_kernel(const FrameArgs a)
{
    int j = 0;
    while (j + 1 < a.njobs && (int)blockIdx.x >= a.first_block[j + 1]) ++j;
    const FrameJob& q = a.job[j];
    const int64_t e = (int64_t)((int)blockIdx.x - a.first_block[j]) * 256 + threadIdx.x;
    if (q.path == kPlanar) frame_job<kPlanar>(q, e);
    else if (q.path == kChannelsLast) frame_job<kChannelsLast>(q, e);
    else frame_job<kStrided>(q, e);
}

} // namespace

extern "C" int p3d_frame_finish(const p3d_frame_job* jobs_host, int32_t n_jobs, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(jobs_host && n_jobs >= 1 && n_jobs <= kMaxJobs, "frame_finish: 1 .. %d jobs", kMaxJobs);
    FrameArgs a{};
    a.njobs = n_jobs;
    int64_t blocks = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const p3d_frame_job& p = jobs_host[j];
        FrameJob& q = a.job[j];
        P3D_REQUIRE(p.src && p.dst, "frame_finish: null pointer in job %d", j);
        P3D_REQUIRE(p.n >= 1 && p.h >= 1 && p.w >= 1 && p.x0 >= 0 && p.y0 >= 0, "frame_finish: job %d: bad sizes", j);
        P3D_REQUIRE(p.mode == P3D_FRAME_SCALE || p.mode == P3D_FRAME_LABEL, "frame_finish: job %d: mode must be SCALE (0) or LABEL (1)", j);
        if (p.mode == P3D_FRAME_SCALE) {
            P3D_REQUIRE(p.c == 1 || p.c == 3, "frame_finish: job %d: SCALE takes 1 or 3 channels (got %d)", j, p.c);
            P3D_REQUIRE(p.dst_bpp == p.c, "frame_finish: job %d: SCALE writes one byte per channel (c = %d, dst_bpp = %d)", j, p.c, p.dst_bpp);
            P3D_REQUIRE(!p.dst_index, "frame_finish: job %d: dst_index belongs to LABEL jobs", j);
        } else {
            P3D_REQUIRE(p.c >= 2 && p.c <= 64, "frame_finish: job %d: LABEL takes 2 .. 64 channels (got %d)", j, p.c);
            P3D_REQUIRE(p.dst_bpp == 3, "frame_finish: job %d: LABEL writes 3-byte palette colours", j);
        }
        P3D_REQUIRE(((int64_t)p.x0 + p.w) * p.dst_bpp <= p.dst_row_pitch, "frame_finish: job %d: the destination rectangle leaves its row pitch", j);
        P3D_REQUIRE(p.n == 1 || ((int64_t)p.y0 + p.h) * p.dst_row_pitch <= p.dst_frame_pitch, "frame_finish: job %d: the destination rectangle leaves its frame pitch", j);
        if (p.dst_index) {
            P3D_REQUIRE((int64_t)p.x0 + p.w <= p.index_row_pitch, "frame_finish: job %d: the index rectangle leaves its row pitch", j);
            P3D_REQUIRE(p.n == 1 || ((int64_t)p.y0 + p.h) * p.index_row_pitch <= p.index_frame_pitch, "frame_finish: job %d: the index rectangle leaves its frame pitch", j);
        }
        for (int t = 0; t < 4; ++t) P3D_REQUIRE(p.src_stride[t] >= 0, "frame_finish: job %d: negative source stride", j);
        q.src = p.src; q.sn = p.src_stride[0]; q.sc = p.src_stride[1]; q.sy = p.src_stride[2]; q.sx = p.src_stride[3];
        q.drow = p.dst_row_pitch; q.dframe = p.dst_frame_pitch;
        q.dst = p.dst + (int64_t)p.y0 * p.dst_row_pitch + (int64_t)p.x0 * p.dst_bpp;
        q.irow = p.index_row_pitch; q.iframe = p.index_frame_pitch;
        q.idx = p.dst_index ? p.dst_index + (int64_t)p.y0 * p.index_row_pitch + p.x0 : nullptr;
        q.pal_dev = p.palette_dev;
        q.mode = p.mode; q.N = p.n; q.C = p.c; q.H = p.h; q.W = p.w; q.bpp = p.dst_bpp;
        q.lo = p.lo; q.scale = p.scale;
        q.groups = (p.w + 3) / 4 + 1;
        for (int k = 0; k < 64; ++k) q.pal[k] = (unsigned)p.palette[3 * k] | ((unsigned)p.palette[3 * k + 1] << 8) | ((unsigned)p.palette[3 * k + 2] << 16);
        const uintptr_t sp = (uintptr_t)p.src;
        P3D_REQUIRE((sp & 3u) == 0, "frame_finish: job %d: src is not aligned to a float", j);
        if (q.sx == 1) {                                     // planar: 16-byte loads when the channel planes keep a group's alignment
            q.path = kPlanar;
            q.vec = q.sc % 4 == 0 ? 4 : 1;                   // (the kernel tests each group's own address)
        } else if (q.sc == 1 || p.c == 1) {                  // channels-last: the widest load that pointer, strides and channel count allow
            q.path = kChannelsLast;
            q.vec = 1;
            for (int v = 2; v <= 4; v *= 2)
                if (sp % (4u * v) == 0 && q.sn % v == 0 && q.sy % v == 0 && q.sx % v == 0 && p.c % 2 == 0 && p.c >= v) q.vec = v;
            if (p.c == 1) q.sc = 1;
        } else {
            q.path = kStrided;
            q.vec = 1;
        }
        a.first_block[j] = (int)blocks;
        blocks += ((int64_t)p.n * p.h * q.groups + 255) / 256;
        P3D_REQUIRE(blocks < (1ll << 31), "frame_finish: too many pixels");
    }
    a.first_block[n_jobs] = (int)blocks;
    hipLaunchKernelGGL(frame_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    count_launch(FAM_AUX);
    return check_launch("frame_finish");
}
