// The entropy decoder of ONE restart interval of a baseline JPEG scan (p3d_video.h states the rules under "the way back from a file"; DESIGN.md section
// 2.1y).  Plain C++ without a library call, for the host and the device alike: video_jpeg_read.hip runs it once per lane, tools/jpeg_unscan_check.cpp
// runs the same text under the host sanitizers.  The bytes did not come from us, so nothing here trusts them — or the tables:
//   * a byte is read only at begin <= p < end; past the end the reader supplies zero bits and the status says so;
//   * every loop has a bound of its own: 16 bits a code, positions <= 63, the blocks of the interval, the bytes of the interval;
//   * a symbol is looked up at an index checked against the table's 256 values, a coefficient stored at a block checked against the frame's.
#ifndef P3D_VIDEO_JPEG_ENTROPY_H
#define P3D_VIDEO_JPEG_ENTROPY_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define P3D_JPEG_HD __host__ __device__ inline
#else
#define P3D_JPEG_HD inline
#endif

namespace p3d {
namespace jpeg {

constexpr int kLookupBits = 8;                      // P3D_VIDEO_JPEG_LOOKUP_BITS
constexpr int kLookup = 1 << kLookupBits;
constexpr int kTableWords = kLookup + 16 + 16 + 64; // P3D_VIDEO_JPEG_TABLE_WORDS: lookup, limit, offset, the 256 values four to a word
enum Status { kNoCode = 1, kRun = 2, kSize = 4, kExhausted = 8, kLeftover = 16 };      // P3D_VIDEO_JPEG_STATUS_*

// The bits of an interval, most significant first.  `acc` holds `n` of them from its top; the last `fake` of those are zeros made up past the end.
struct Bits {
    const uint8_t* data; int64_t p, end;
    uint32_t acc; int n, fake, status;

    P3D_JPEG_HD int byte()                          // the next data byte: a 0x00 after a 0xFF is stuffing and goes with it
    {
        const int b = data[p++];
        if (b == 0xFF && p < end && data[p] == 0) ++p;
        return b;
    }
    P3D_JPEG_HD void fill()                         // to at least 25 bits
    {
        while (n <= 24) {
            uint32_t b = 0;
            if (p < end) b = (uint32_t)byte(); else fake += 8;
            acc |= b << (24 - n);
            n += 8;
        }
    }
    P3D_JPEG_HD uint32_t peek16() const { return acc >> 16; }
    P3D_JPEG_HD void take(int k)                    // 0 <= k <= 16 <= n
    {
        acc = k ? acc << k : acc;
        n -= k;
        if (n < fake) { fake = n; status |= kExhausted; }
    }
    P3D_JPEG_HD int whole_bytes_left()              // data bytes nobody read: those in `acc` and those never fetched
    {
        int rest = (n - fake) >> 3;
        while (p < end) { byte(); if (rest < 2) ++rest; }
        return rest;
    }
};

// One Huffman symbol under `table` (kTableWords words: jpeg_decode_tables' format), or -1 with the status set.  A code of up to kLookupBits bits is one
// read; a longer one walks the lengths as Annex F.2.2.3 does: the first length whose prefix is below limit[length] (= maxcode + 1; 0: no code).
P3D_JPEG_HD int symbol(Bits& s, const uint32_t* table)
{
    s.fill();
    const uint32_t peek = s.peek16();
    const uint32_t e = table[peek >> (16 - kLookupBits)];
    int length = (int)(e >> 16), value = (int)(e & 255u);
    if (length < 1 || length > kLookupBits) {
        value = -1;
        for (length = kLookupBits + 1; length <= 16; ++length) {
            const uint32_t code = peek >> (16 - length);
            if (code < table[kLookup + length - 1]) {
                const int64_t at = (int64_t)code + (int32_t)table[kLookup + 16 + length - 1];
                if (at >= 0 && at < 256) value = (int)((table[kLookup + 32 + (at >> 2)] >> (8 * (at & 3))) & 255u);
                break;
            }
        }
        if (value < 0) { length = 16; s.status |= kNoCode; }
    }
    s.take(length);
    return s.status ? -1 : value;
}

// The `size` extra bits of a value (1 <= size <= 11), extended as F.2.2.1 does: a leading 1 is the value, a leading 0 the value - 2^size + 1.
P3D_JPEG_HD int extra(Bits& s, int size)
{
    s.fill();
    const int v = (int)(s.peek16() >> (16 - size));
    s.take(size);
    return v >= (1 << (size - 1)) ? v : v - (1 << size) + 1;
}

// Decodes the interval data[begin, end) of `n_mcus` MCUs into `frame` (the frame's coefficients, zeroed by the caller: only non-zero values are stored),
// whose first MCU is `mcu0`.  `bpm` blocks an MCU in the output (3 or 6), `coded` of them in the stream (bpm, or 1: a grey stream codes Y alone).
// `tables`: DC luma, DC chroma, AC luma, AC chroma.  Returns the status bits; on the first of them the interval ends where it stands.
P3D_JPEG_HD int unscan_interval(const uint8_t* data, int64_t begin, int64_t end, const uint32_t* tables, int bpm, int coded, int mcu0, int n_mcus,
                                int64_t frame_blocks, int16_t* frame)
{
    Bits s = {data, begin, end < begin ? begin : end, 0u, 0, 0, 0};
    int pred[3] = {0, 0, 0};
    for (int m = 0; m < n_mcus; ++m) {
        for (int k = 0; k < coded; ++k) {
            const int comp = bpm == 3 ? k : (k < 4 ? 0 : k - 3);
            const uint32_t* const dc = tables + (comp ? kTableWords : 0);
            const uint32_t* const ac = tables + (comp ? 3 : 2) * kTableWords;
            const int64_t block = ((int64_t)mcu0 + m) * bpm + k;
            int16_t* const out = frame + block * 64;
            const bool inside = block >= 0 && block < frame_blocks;

            const int size = symbol(s, dc);
            if (s.status) return s.status;
            if (size > 11) return s.status | kSize;
            const int diff = size ? extra(s, size) : 0;
            if (s.status) return s.status;
            const int v = pred[comp] + diff;
            pred[comp] = v < -32768 ? -32768 : (v > 32767 ? 32767 : v);
            if (inside && pred[comp]) out[0] = (int16_t)pred[comp];

            for (int z = 1; z < 64;) {
                const int rs = symbol(s, ac);
                if (s.status) return s.status;
                const int run = rs >> 4, bits = rs & 15;
                if (bits == 0) {
                    if (run == 0) break;                                        // EOB
                    if (run != 15) return s.status | kSize;                     // EOBn belongs to progressive scans
                    z += 16;                                                    // ZRL: a value must follow
                    if (z > 63) return s.status | kRun;
                    continue;
                }
                if (bits > 10) return s.status | kSize;
                const int value = extra(s, bits);
                if (s.status) return s.status;
                z += run;
                if (z > 63) return s.status | kRun;
                if (inside) out[z] = (int16_t)value;
                ++z;
            }
        }
    }
    return s.whole_bytes_left() > 1 ? s.status | kLeftover : s.status;
}

} // namespace jpeg
} // namespace p3d
#endif
