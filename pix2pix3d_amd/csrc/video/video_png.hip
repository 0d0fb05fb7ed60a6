// Lossless frames: the zlib streams of PNG and APNG files (p3d_video.h; pix2pix3d_amd/video/png.py).  Integer rules throughout: every
// byte is defined by the header, and the formulations of video/png.py produce the same bytes.
//
// p3d_video_png_filter  a wave owns one row: a first pass sums |residual| of the five filter types (adaptive only), a wave reduction picks the type, a
//                       second pass stores the residuals.  Four rows a work-group; the row above is read again rather than kept.
// p3d_video_png_count   a work-group of ONE wave owns a segment and walks it 64 bytes a step.  A ballot of the run starts gives every byte its place k in
//                       its run (the length of the run left open by the steps before is the only thing carried), and k and "is the next byte another"
//                       decide the byte's token (token_of): no lane ever loops over a run.  Symbol counts gather in LDS, the rest in registers.
// p3d_video_png_emit    the same walk; every lane turns its token into at most 30 bits, a wave prefix sum places them, they are ORed into a window of LDS
//                       words, and the whole words of the window leave after every step — as 32-bit stores where the segment starts on a word of the
//                       output, as bytes otherwise.  The frame's header bits go first, 64 words a step, through the same window.
#include "../p3d_common.h"
#include "p3d_video.h"

namespace {

using namespace p3d;

constexpr int kSymbols = P3D_VIDEO_PNG_SYMBOLS, kStats = P3D_VIDEO_PNG_STATS, kHeaderWords = P3D_VIDEO_PNG_HEADER_WORDS;
constexpr int kMaxMatch = 258;
constexpr unsigned kAdler = 65521u;
constexpr int kWindow = 68;                                                   // words: 31 bits left over + 64 lanes x 32 bits = 65 words, and the one an OR may spill into
static_assert(kStats == kSymbols + 4, "a segment's record: the counts, extra bits, matches, s1, s2");

// ---- filter ------------------------------------------------------------------------------------------------------------------------------------
struct FilterArgs {
    const uint8_t* frames; int64_t frame_pitch, row_pitch;
    int H, n, bpp, filter;                                                    // n: bytes of a row of pixels
    int64_t rows;                                                             // of the clip
    uint8_t* out;
};

__device__ __forceinline__ int paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int predictor(int type, int a, int b, int c)
{
    return type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
}

__global__ void __launch_bounds__(256) png_filter_kernel(const FilterArgs a)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= a.rows) return;                                                // (no barrier below)
    const int64_t f = row / a.H;
    const int y = (int)(row - f * a.H);
    const uint8_t* const cur = a.frames + f * a.frame_pitch + (int64_t)y * a.row_pitch;
    const uint8_t* const up = cur - a.row_pitch;                              // read only where y > 0
    int type = a.filter;
    if (type == P3D_VIDEO_PNG_ADAPTIVE) {
        unsigned long long sums[5] = {0, 0, 0, 0, 0};
        for (int i = lane; i < a.n; i += kWave) {
            const int x = cur[i], left = i >= a.bpp ? cur[i - a.bpp] : 0, above = y ? up[i] : 0, corner = y && i >= a.bpp ? up[i - a.bpp] : 0;
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                const int r = (x - predictor(t, left, above, corner)) & 255;
                sums[t] += (unsigned)(r < 128 ? r : 256 - r);
            }
        }
        type = 0;
        unsigned long long best = 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            unsigned long long s = sums[t];
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) s += __shfl_xor(s, d);
            if (t == 0 || s < best) { best = s; type = t; }                   // strictly smaller: a tie stays with the lower type
        }
    }
    uint8_t* const out = a.out + row * ((int64_t)a.n + 1);
    if (lane == 0) out[0] = (uint8_t)type;
    for (int i = lane; i < a.n; i += kWave) {
        const int x = cur[i], left = i >= a.bpp ? cur[i - a.bpp] : 0, above = y ? up[i] : 0, corner = y && i >= a.bpp ? up[i - a.bpp] : 0;
        out[1 + i] = (uint8_t)(x - predictor(type, left, above, corner));
    }
}

// ---- the walk over a segment both coders share -------------------------------------------------------------------------------------------------------
struct SegArgs {
    const uint8_t* filtered;
    int H, R, segment_rows, n_segments;                                        // R: bytes of a filtered row; segments of a frame
};

struct Segment { const uint8_t* bytes; int L; int64_t frame; int index; };

__device__ __forceinline__ Segment segment_of(const SegArgs& a, unsigned group)
{
    Segment s;
    s.frame = group / (unsigned)a.n_segments;
    s.index = (int)(group - s.frame * a.n_segments);
    const int row0 = s.index * a.segment_rows;                                // (n_segments = ceil(H / segment_rows): row0 < H)
    s.L = min(a.segment_rows, a.H - row0) * a.R;                              // < 2^31 by the entry point's check
    s.bytes = a.filtered + (s.frame * a.H + row0) * (int64_t)a.R;
    return s;
}

struct Step { unsigned byte; int k; bool valid, last; };                      // a lane's byte, its place in its run, and whether the run ends with it

// The 64 bytes from `base` on.  `open` is the length of the run that reaches `base` from the steps before (0 at the segment's start) and is updated.
__device__ __forceinline__ Step walk(const Segment& s, int base, int lane, int& open)
{
    Step t;
    const int i = base + lane;
    t.valid = i < s.L;
    t.byte = t.valid ? s.bytes[i] : 0x100u;                                   // past the end: no byte's equal
    unsigned prev = __shfl_up(t.byte, 1), next = __shfl_down(t.byte, 1);
    if (lane == 0) prev = base ? s.bytes[base - 1] : 0x100u;
    if (lane == kWave - 1) next = i + 1 < s.L ? s.bytes[i + 1] : 0x100u;
    t.last = t.byte != next;
    const unsigned long long starts = __ballot(t.valid && t.byte != prev);
    const unsigned long long upto = starts & (~0ull >> (kWave - 1 - lane));    // the starts at or before this lane
    t.k = upto ? lane - (63 - __clzll(upto)) : open + lane;
    open = starts ? kWave - (63 - __clzll(starts)) : open + kWave;             // (only a full step is followed by another)
    return t;
}

struct Token { int literals, length; };                                       // of the lane's byte: 0, 1 or 2 literals of it, or a match of `length` (0: none)

__device__ __forceinline__ Token token_of(const Step& t)
{
    Token k = {0, 0};
    if (!t.valid) return k;
    if (t.k == 0) { k.literals = 1; return k; }
    const int r = t.k % kMaxMatch;                                            // t.k: the bytes of the run after its first, up to this one
    if (r == 0) k.length = kMaxMatch;
    else if (t.last) { if (r >= 3) k.length = r; else k.literals = r; }
    return k;
}

__device__ __forceinline__ void length_symbol(int length, int& symbol, int& extra_bits, int& extra)
{
    const int v = length - 3;
    extra_bits = 0; extra = 0;
    if (length == kMaxMatch) { symbol = 285; return; }
    if (v < 8) { symbol = 257 + v; return; }
    extra_bits = 29 - __clz(v);                                               // floor(log2 v) - 2
    symbol = 261 + 4 * extra_bits + ((v >> extra_bits) & 3);
    extra = v & ((1 << extra_bits) - 1);
}

template <class T> __device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

// ---- count ---------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWave) png_count_kernel(const SegArgs a, int32_t* const stats)
{
    __shared__ int counts[kSymbols];
    const int lane = threadIdx.x;
    for (int i = lane; i < kSymbols; i += kWave) counts[i] = 0;
    __syncthreads();
    const Segment s = segment_of(a, blockIdx.x);
    int open = 0, extra_bits = 0, matches = 0;
    unsigned long long s1 = 0, s2 = 0;
    for (int base = 0; base < s.L; base += kWave) {
        const Step t = walk(s, base, lane, open);
        const Token k = token_of(t);
        if (k.literals) atomicAdd(&counts[t.byte], k.literals);
        if (k.length) {
            int symbol, e, v;
            length_symbol(k.length, symbol, e, v);
            atomicAdd(&counts[symbol], 1);
            extra_bits += e; ++matches;
        }
        if (t.valid) {
            s1 += t.byte;
            s2 += (unsigned long long)((unsigned)(s.L - (base + lane)) % kAdler) * t.byte;      // < 2^24 a byte, fewer than 2^25 bytes a lane
        }
    }
    extra_bits = wave_sum(extra_bits); matches = wave_sum(matches);
    s1 = wave_sum(s1); s2 = wave_sum(s2);
    __syncthreads();
    int32_t* const out = stats + (int64_t)blockIdx.x * kStats;
    for (int i = lane; i < kSymbols; i += kWave) out[i] = counts[i];
    if (lane == 0) {
        out[kSymbols] = extra_bits; out[kSymbols + 1] = matches;
        out[kSymbols + 2] = (int32_t)(s1 % kAdler); out[kSymbols + 3] = (int32_t)(s2 % kAdler);
    }
}

// ---- emit ----------------------------------------------------------------------------------------------------------------------------------------
struct EmitArgs {
    SegArgs g;
    const uint32_t* tables; const uint32_t* headers; const int32_t* header_bits; const uint32_t* adler; const int64_t* offsets;
    uint8_t* data; int64_t data_bytes;
};

// The segment's bit string on its way out: win[0 ..] holds the bits from the byte `at` of the output on, `bit` of them so far; at most 31 stay behind
// after a put.
struct Writer {
    unsigned* win; int bit; int64_t at;
    uint8_t* data; int64_t data_bytes; bool words;                            // words: `at` stays on a 4-byte boundary of the output
};

__device__ __forceinline__ void store_byte(const Writer& w, int64_t pos, unsigned v)
{
    if (pos >= 0 && pos < w.data_bytes) w.data[pos] = (uint8_t)v;
}

// Every lane appends the low n (0 .. 32) bits of v, lane after lane; then the whole words of the window leave.  Called by the whole wave.
__device__ __forceinline__ void put(Writer& w, unsigned v, int n, int lane)
{
    int end = n;                                                              // inclusive prefix sum over the wave
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int t = __shfl_up(end, d);
        if (lane >= d) end += t;
    }
    const int total = __shfl(end, kWave - 1);
    if (n) {
        const int first = w.bit + end - n;                                    // < 31 + 64 * 32
        const unsigned long long t = (unsigned long long)(n < 32 ? v & ((1u << n) - 1u) : v) << (first & 31);
        atomicOr(&w.win[first >> 5], (unsigned)t);
        if ((unsigned)(t >> 32)) atomicOr(&w.win[(first >> 5) + 1], (unsigned)(t >> 32));
    }
    w.bit += total;
    const int full = w.bit >> 5;                                              // 0 .. 64, the same in every lane
    if (full == 0) return;                                                    // (the next put's ORs touch only words this wave's own lanes wrote: a barrier at the next flush orders them)
    __syncthreads();
    const unsigned word = w.win[lane], rest = w.win[full];
    if (lane < full) {
        const int64_t pos = w.at + 4 * (int64_t)lane;
        if (w.words && pos + 4 <= w.data_bytes) {
            *(unsigned*)(w.data + pos) = word;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) store_byte(w, pos + j, word >> (8 * j));
        }
    }
    __syncthreads();
    w.win[lane] = lane == 0 ? rest : 0u;
    if (lane < kWindow - kWave) w.win[kWave + lane] = 0u;
    __syncthreads();
    w.at += 4 * (int64_t)full; w.bit &= 31;
}

__global__ void __launch_bounds__(kWave) png_emit_kernel(const EmitArgs a)
{
    __shared__ unsigned table[kSymbols];
    __shared__ unsigned win[kWindow];
    const int lane = threadIdx.x;
    const Segment s = segment_of(a.g, blockIdx.x);
    for (int i = lane; i < kSymbols; i += kWave) {
        const unsigned e = a.tables[s.frame * kSymbols + i];
        const unsigned len = min(e >> 16, 15u);
        table[i] = len << 16 | (e & ((1u << len) - 1u));                      // whatever the caller's table holds, a token stays within 30 bits
    }
    for (int i = lane; i < kWindow; i += kWave) win[i] = 0u;
    __syncthreads();
    const bool final = s.index == a.g.n_segments - 1;
    Writer w;
    w.win = win; w.bit = 0; w.at = a.offsets[blockIdx.x]; w.data = a.data; w.data_bytes = a.data_bytes;
    w.words = w.at >= 0 && (((uintptr_t)a.data + (uint64_t)w.at) & 3u) == 0;
    if (lane == 0 && s.index == 0) { store_byte(w, w.at - 2, 0x78); store_byte(w, w.at - 1, 0x01); }

    put(w, final ? 1u : 0u, lane == 0 ? 1 : 0, lane);                          // BFINAL
    const int header_bits = min(max(a.header_bits[s.frame], 0), 32 * kHeaderWords);
    const uint32_t* const header = a.headers + s.frame * kHeaderWords;
    for (int base = 0; base < header_bits; base += 32 * kWave) {
        const int n = min(max(header_bits - base - 32 * lane, 0), 32);
        put(w, n ? header[(base >> 5) + lane] : 0u, n, lane);
    }
    int open = 0;
    for (int base = 0; base < s.L; base += kWave) {
        const Step t = walk(s, base, lane, open);
        const Token k = token_of(t);
        unsigned v = 0; int n = 0;
        if (k.literals) {
            const unsigned e = table[t.byte], len = e >> 16, code = e & 0xFFFFu;
            v = code; n = (int)len;
            if (k.literals == 2) { v |= code << len; n += (int)len; }
        } else if (k.length) {
            int symbol, eb, ev;
            length_symbol(k.length, symbol, eb, ev);
            const unsigned e = table[symbol], len = e >> 16;
            v = (e & 0xFFFFu) | (unsigned)ev << len;                          // the code, its extra bits, and the distance code: one 0 bit
            n = (int)len + eb + 1;
        }
        put(w, v, n, lane);
    }
    const unsigned eob = table[256];
    put(w, eob & 0xFFFFu, lane == 0 ? (int)(eob >> 16) : 0, lane);
    if (final) {
        put(w, 0u, lane == 0 ? (-w.bit) & 7 : 0, lane);
    } else {
        put(w, 0u, lane == 0 ? 3 + ((-(w.bit + 3)) & 7) : 0, lane);             // the stored block's BFINAL, BTYPE, and zeros up to the byte
        put(w, 0xFFFF0000u, lane == 0 ? 32 : 0, lane);                          // LEN = 0, NLEN = 0xFFFF
    }
    __syncthreads();
    if (lane == 0) {                                                            // w.bit is 0, 8, 16 or 24: the bytes of the last, partial word
        const int rest = w.bit >> 3;
        for (int j = 0; j < rest; ++j) store_byte(w, w.at + j, win[0] >> (8 * j));
        if (final) {
            const unsigned sum = a.adler[s.frame];
            for (int j = 0; j < 4; ++j) store_byte(w, w.at + rest + j, sum >> (24 - 8 * j));
        }
    }
}

// The checks count and emit share.  *groups: the segments of the clip, 0 when there is nothing to code.
int geometry(const char* what, int32_t n_frames, int32_t h, int32_t row_bytes, int32_t segment_rows, SegArgs* g, int64_t* groups)
{
    P3D_REQUIRE(n_frames >= 0 && h >= 0 && row_bytes >= 0, "%s: n_frames, h and row_bytes must be >= 0 (got %d, %d, %d)", what, n_frames, h, row_bytes);
    P3D_REQUIRE(segment_rows >= 1, "%s: segment_rows must be >= 1 (got %d)", what, segment_rows);
    const int64_t frame = (int64_t)h * row_bytes;
    P3D_REQUIRE(frame < (1ll << 31) && frame * n_frames < (1ll << 31), "%s: %d x %d x %d filtered bytes reach 2^31", what, n_frames, h, row_bytes);
    g->H = h; g->R = row_bytes; g->segment_rows = min(segment_rows, max(h, 1));
    g->n_segments = (h + g->segment_rows - 1) / g->segment_rows;
    *groups = row_bytes <= 1 ? 0 : (int64_t)n_frames * g->n_segments;
    return P3D_OK;
}

} // namespace

extern "C" int p3d_video_png_filter(const uint8_t* frames, int64_t frame_pitch, int64_t row_pitch, int32_t n_frames, int32_t h, int32_t w, int32_t bpp,
                                    int32_t filter, uint8_t* filtered, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(n_frames >= 0 && h >= 0 && w >= 0, "video_png_filter: n_frames, h and w must be >= 0 (got %d, %d, %d)", n_frames, h, w);
    P3D_REQUIRE(bpp >= 1 && bpp <= 4, "video_png_filter: bpp must be 1 .. 4 (got %d)", bpp);
    P3D_REQUIRE(filter >= 0 && filter <= P3D_VIDEO_PNG_ADAPTIVE, "video_png_filter: filter must be 0 .. 5 (got %d)", filter);
    const int64_t n = (int64_t)w * bpp, frame = (int64_t)h * (n + 1);
    P3D_REQUIRE(n < (1ll << 31) && frame < (1ll << 31) && frame * n_frames < (1ll << 31), "video_png_filter: %d x %d x %d pixels of %d bytes reach 2^31",
                n_frames, h, w, bpp);
    const int64_t rows = (int64_t)n_frames * h;
    if (rows * w == 0) return P3D_OK;
    P3D_REQUIRE(frames && filtered, "video_png_filter: frames and filtered must be non-null");
    P3D_REQUIRE(row_pitch >= n && frame_pitch >= 0, "video_png_filter: the row pitch is shorter than the row, or the frame pitch negative");
    FilterArgs a;
    a.frames = frames; a.frame_pitch = frame_pitch; a.row_pitch = row_pitch; a.H = h; a.n = (int)n; a.bpp = bpp; a.filter = filter; a.rows = rows;
    a.out = filtered;
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    count_launch(FAM_AUX);
    return check_launch("video_png_filter");
}

extern "C" int p3d_video_png_count(const uint8_t* filtered, int32_t n_frames, int32_t h, int32_t row_bytes, int32_t segment_rows, int32_t* stats,
                                   p3d_stream_t stream)
{
    using namespace p3d;
    SegArgs g;
    int64_t groups = 0;
    const int rc = geometry("video_png_count", n_frames, h, row_bytes, segment_rows, &g, &groups);
    if (rc != P3D_OK) return rc;
    if (groups == 0) return P3D_OK;
    P3D_REQUIRE(filtered && stats && ((uintptr_t)stats & 3u) == 0, "video_png_count: filtered and stats must be non-null, stats 4-byte aligned");
    g.filtered = filtered;
    hipLaunchKernelGGL(png_count_kernel, dim3((unsigned)groups), dim3(kWave), 0, (hipStream_t)stream, g, stats);
    count_launch(FAM_AUX);
    return check_launch("video_png_count");
}

extern "C" int p3d_video_png_emit(const uint8_t* filtered, int32_t n_frames, int32_t h, int32_t row_bytes, int32_t segment_rows, const uint32_t* tables,
                                  const uint32_t* headers, const int32_t* header_bits, const uint32_t* adler, const int64_t* offsets, uint8_t* data,
                                  int64_t data_bytes, p3d_stream_t stream)
{
    using namespace p3d;
    EmitArgs a;
    int64_t groups = 0;
    const int rc = geometry("video_png_emit", n_frames, h, row_bytes, segment_rows, &a.g, &groups);
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(data_bytes >= 0, "video_png_emit: data_bytes must be >= 0 (got %lld)", (long long)data_bytes);
    if (groups == 0) return P3D_OK;
    P3D_REQUIRE(filtered && data, "video_png_emit: filtered and data must be non-null");
    P3D_REQUIRE(tables && headers && header_bits && adler && (((uintptr_t)tables | (uintptr_t)headers | (uintptr_t)header_bits | (uintptr_t)adler) & 3u) == 0,
                "video_png_emit: tables, headers, header_bits and adler must be non-null and 4-byte aligned");
    P3D_REQUIRE(offsets && ((uintptr_t)offsets & 7u) == 0, "video_png_emit: offsets must be non-null and 8-byte aligned");
    a.g.filtered = filtered; a.tables = tables; a.headers = headers; a.header_bits = header_bits; a.adler = adler; a.offsets = offsets;
    a.data = data; a.data_bytes = data_bytes;
    hipLaunchKernelGGL(png_emit_kernel, dim3((unsigned)groups), dim3(kWave), 0, (hipStream_t)stream, a);
    count_launch(FAM_AUX);
    return check_launch("video_png_emit");
}
