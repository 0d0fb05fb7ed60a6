// RFC 1951 inflate of ONE part of a deflate stream (p3d_video.h states the rules under "the way back from a lossless file").
// Plain C++ without a library call, for the host and the device alike: video_png_read.hip runs it once per lane, tools/png_inflate_check.cpp runs the
// same text under the host sanitizers.  The bytes did not come from us, so nothing here trusts them:
//   * a byte is read only at in_begin <= p < in_end; past the end the reader supplies zero bits and the status says so;
//   * a byte is stored only at out_begin <= q < out_end, and a match reads only what the part itself has stored;
//   * every loop has a bound of its own: 15 bits a code, 19 + 316 code lengths, 258 bytes a match, 65535 bytes a stored block, and a block loop and a
//     symbol loop that consume at least one bit a turn and end with the first bit read past the end;
//   * a decode table is indexed below its size whatever the lengths hold: symbol[] by an index < the number of symbols, count[] by a length <= 15.
// The decode state of a part — the code lengths and the canonical decode tables of the literal/length and the distance code (per length the number of
// codes, and the symbols in code order: zlib's puff.c has the same form) — lives where the caller puts it: `State` holds pointers and a stride, so that
// the kernel can interleave the lanes of a work-group in LDS and the host program can pass a plain array (stride 1).  kStateHalves 16-bit words a part.
#ifndef P3D_VIDEO_PNG_INFLATE_H
#define P3D_VIDEO_PNG_INFLATE_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define P3D_PNG_HD __host__ __device__ inline
#else
#define P3D_PNG_HD inline
#endif

namespace p3d {
namespace png {

enum Status {                                       // P3D_VIDEO_PNG_STATUS_*
    kBlockType = 1, kStored = 2, kCodeLengths = 4, kNoCode = 8, kDistance = 16, kOverflow = 32, kExhausted = 64, kLeftover = 128, kBoundary = 256,
    kShort = 512, kFilter = 1024, kAdler = 2048
};
constexpr int kMaxBits = 15, kLitCodes = 288, kDistCodes = 32, kMaxLit = 286, kMaxDist = 30;
// 16-bit words of a part's state: count[2][16], next[16] (the running offsets while a table is made), symbol[288 + 32], and 320 code lengths, one a
// word's half: 32 + 16 + 320 + 160 = 528 words of 16 bits, 1056 bytes.
constexpr int kCountAt = 0, kNextAt = 32, kSymbolAt = 48, kLengthAt = 368, kStateHalves = 528;

struct State {
    uint16_t* base; int stride;                     // word i of this part's state is base[i * stride]
    P3D_PNG_HD uint16_t& at(int i) const { return base[(int64_t)i * stride]; }
    P3D_PNG_HD int length(int i) const { return (at(kLengthAt + (i >> 1)) >> (8 * (i & 1))) & 255; }
    P3D_PNG_HD void set_length(int i, int v) const
    {
        uint16_t& w = at(kLengthAt + (i >> 1));
        w = (uint16_t)((i & 1) ? (w & 0x00FF) | (v << 8) : (w & 0xFF00) | v);
    }
};

// The bits of a part, least significant first.  `acc` holds `n` of them from its bottom; the top `fake` of those are zeros made up past the end.
struct Bits {
    const uint8_t* data; int64_t p, end;
    uint64_t acc; int n, fake, status;

    P3D_PNG_HD void fill()                          // to at least 32 bits: four bytes at once while the part has them (one wait for four loads), else to 57
    {
        if (n > 32) return;
        if (p + 4 <= end) {
            const uint64_t w = (uint64_t)data[p] | (uint64_t)data[p + 1] << 8 | (uint64_t)data[p + 2] << 16 | (uint64_t)data[p + 3] << 24;
            acc |= w << n;
            n += 32; p += 4;
            return;
        }
        while (n <= 56) {
            uint64_t b = 0;
            if (p < end) b = data[p++]; else fake += 8;
            acc |= b << n;
            n += 8;
        }
    }
    P3D_PNG_HD void take(int k)                     // 0 <= k <= 32 <= n
    {
        acc >>= k;
        n -= k;
        if (n < fake) { fake = n; status |= kExhausted; }
    }
    P3D_PNG_HD uint32_t bits(int k)                 // the next k bits, 0 <= k <= 32
    {
        fill();
        const uint32_t v = (uint32_t)(acc & ((1ull << k) - 1ull));
        take(k);
        return v;
    }
    P3D_PNG_HD int64_t real_bits_left() const { return 8 * (end - p) + (n - fake); }
    P3D_PNG_HD void to_byte() { take((n - fake) & 7); }      // (real bits and made-up bits are whole bytes apart)
    P3D_PNG_HD void rewind()                        // the whole bytes in `acc` go back: a stored block is read from `data` itself
    {
        p -= (n - fake) >> 3;
        acc = 0; n = 0; fake = 0;
    }
};

// The canonical decode table of the code whose lengths are s.length(first .. first + n - 1): count[which][l] codes of length l, symbol[] in code order.
// False for an over-subscribed code; an incomplete one is accepted.
P3D_PNG_HD bool construct(const State& s, int which, int first, int n)
{
    const int count = kCountAt + 16 * which, symbol = kSymbolAt + (which ? kLitCodes : 0);
    for (int l = 0; l <= kMaxBits; ++l) s.at(count + l) = 0;
    for (int i = 0; i < n; ++i) {
        const int l = s.length(first + i) & kMaxBits;
        s.at(count + l) = (uint16_t)(s.at(count + l) + 1);
    }
    int left = 1, offset = 0;
    for (int l = 1; l <= kMaxBits; ++l) {
        left = 2 * left - (int)s.at(count + l);
        if (left < 0) return false;
        s.at(kNextAt + l) = (uint16_t)offset;
        offset += s.at(count + l);
    }
    for (int i = 0; i < n; ++i) {
        const int l = s.length(first + i) & kMaxBits;
        if (l) {
            const int k = s.at(kNextAt + l);                                      // < n: the offsets add up to the symbols that have a code
            s.at(kNextAt + l) = (uint16_t)(k + 1);
            if (k < n) s.at(symbol + k) = (uint16_t)i;
        }
    }
    return true;
}

// One symbol under the table `which`, or -1 with the status set: the first length l whose l-bit prefix, read as a canonical code, lies among the codes
// of that length.  No such l within 15 bits: NO_CODE, and 15 bits count as read.
P3D_PNG_HD int symbol(Bits& b, const State& s, int which)
{
    const int count = kCountAt + 16 * which, table = kSymbolAt + (which ? kLitCodes : 0), size = which ? kDistCodes : kLitCodes;
    b.fill();
    uint32_t peek = (uint32_t)b.acc;
    int code = 0, first = 0, index = 0, value = -1, l = 1;
    for (; l <= kMaxBits; ++l) {
        code |= (int)(peek & 1u);
        peek >>= 1;
        const int c = s.at(count + l);
        if (code - c < first) {
            const int k = index + (code - first);
            if (k >= 0 && k < size) value = s.at(table + k);
            break;
        }
        index += c; first = (first + c) << 1; code <<= 1;
    }
    if (value < 0) { l = kMaxBits; b.status |= kNoCode; }
    b.take(l);
    return b.status ? -1 : value;
}

P3D_PNG_HD int code_length_order(int i)             // RFC 1951 section 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
{
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 |
                        11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// The header of a dynamic block: both tables made, or the status set.
P3D_PNG_HD void dynamic_tables(Bits& b, const State& s)
{
    const int n_lit = (int)b.bits(5) + 257, n_dist = (int)b.bits(5) + 1, n_cl = (int)b.bits(4) + 4;
    if (b.status) return;
    if (n_lit > kMaxLit || n_dist > kMaxDist) { b.status |= kCodeLengths; return; }
    for (int i = 0; i < 19; ++i) s.set_length(code_length_order(i), i < n_cl ? (int)b.bits(3) : 0);
    if (b.status) return;
    if (!construct(s, 1, 0, 19)) { b.status |= kCodeLengths; return; }         // the code-length code borrows the distance table: 19 <= 32 symbols
    const int total = n_lit + n_dist;
    for (int i = 0; i < total;) {                                               // every turn adds at least one length or ends
        const int v = symbol(b, s, 1);
        if (b.status) return;
        if (v < 16) { s.set_length(i++, v); continue; }
        int value = 0, repeat;
        if (v == 16) {
            if (i == 0) { b.status |= kCodeLengths; return; }
            value = s.length(i - 1);
            repeat = 3 + (int)b.bits(2);
        } else if (v == 17) repeat = 3 + (int)b.bits(3);
        else repeat = 11 + (int)b.bits(7);
        if (b.status) return;
        if (i + repeat > total) { b.status |= kCodeLengths; return; }
        for (int k = 0; k < repeat; ++k) s.set_length(i++, value);
    }
    if (!construct(s, 0, 0, n_lit) || !construct(s, 1, n_lit, n_dist)) b.status |= kCodeLengths;
}

P3D_PNG_HD void fixed_tables(const State& s)         // RFC 1951 section 3.2.6
{
    for (int i = 0; i < kLitCodes; ++i) s.set_length(i, i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (int i = 0; i < kDistCodes; ++i) s.set_length(kLitCodes + i, 5);
    construct(s, 0, 0, kLitCodes);
    construct(s, 1, kLitCodes, kDistCodes);
}

// Inflates the part data[in_begin, in_end) into out[out_begin, out_end), which the caller zeroed.  `final`: the part ends with the block whose BFINAL is
// 1; otherwise with the first block that ends on the bit 8 in_end.  Returns the status bits; on the first of them the part ends where it stands.
P3D_PNG_HD int inflate_part(const uint8_t* data, int64_t in_begin, int64_t in_end, uint8_t* out, int64_t out_begin, int64_t out_end, bool final, const State& s)
{
    Bits b = {data, in_begin, in_end < in_begin ? in_begin : in_end, 0ull, 0, 0, 0};
    if (out_end < out_begin) out_end = out_begin;
    int64_t q = out_begin;
    for (;;) {                                                                  // a block reads at least 3 bits: past the end the status ends the loop
        const int last = (int)b.bits(1), type = (int)b.bits(2);
        if (b.status) return b.status;
        if (type == 3) return b.status | kBlockType;
        if (last && !final) return b.status | kBoundary;
        if (type == 0) {
            b.to_byte();
            const uint32_t v = b.bits(32);
            if (b.status) return b.status;
            const int64_t len = v & 0xFFFFu;
            if (len != (int64_t)((~v >> 16) & 0xFFFFu)) return b.status | kStored;
            b.rewind();
            const int64_t have = b.end - b.p, room = out_end - q;
            const int64_t n = len < have ? (len < room ? len : room) : (have < room ? have : room);
            for (int64_t i = 0; i < n; ++i) out[q + i] = data[b.p + i];
            b.p += n; q += n;
            if (n < len) return b.status | (have <= n ? kExhausted : kOverflow);
        } else {
            if (type == 1) fixed_tables(s); else dynamic_tables(b, s);
            if (b.status) return b.status;
            for (;;) {                                                          // a symbol reads at least 1 bit
                const int v = symbol(b, s, 0);
                if (b.status) return b.status;
                if (v < 256) {
                    if (q >= out_end) return b.status | kOverflow;
                    out[q++] = (uint8_t)v;
                    continue;
                }
                if (v == 256) break;
                if (v >= kMaxLit) return b.status | kNoCode;
                const int k = v - 257;                                          // RFC 1951 section 3.2.5, in closed form
                const int le = k < 8 || k == 28 ? 0 : (k - 4) >> 2;
                const int length = k < 8 ? 3 + k : k == 28 ? 258 : 3 + ((4 + (k & 3)) << le) + (int)b.bits(le);
                if (b.status) return b.status;
                const int d = symbol(b, s, 1);
                if (b.status) return b.status;
                if (d >= kMaxDist) return b.status | kNoCode;
                const int de = d < 4 ? 0 : (d >> 1) - 1;
                const int64_t distance = d < 4 ? 1 + d : 1 + ((int64_t)(2 + (d & 1)) << de) + (int64_t)b.bits(de);
                if (b.status) return b.status;
                if (distance > q - out_begin) return b.status | kDistance;
                // Byte by byte, in order: an overlapping match repeats itself.  The bytes go through a register, so that a store never waits for the
                // load of the byte before it: up to 8 source bytes are read at once — all of them written before this turn, since 8 <= distance or the
                // turn reads `distance` bytes — and a match at a distance of up to 8 repeats those for its whole length.
                const int period = distance < 8 ? (int)distance : 8;
                for (int done = 0; done < length;) {
                    uint64_t chunk = 0;
                    for (int j = 0; j < period; ++j) chunk |= (uint64_t)out[q - distance + j] << (8 * j);
                    const int n = distance <= 8 || length - done < 8 ? length - done : 8;
                    for (int j = 0, shift = 0; j < n; ++j) {
                        if (q >= out_end) return b.status | kOverflow;
                        out[q++] = (uint8_t)(chunk >> shift);
                        shift = shift + 8 == 8 * period ? 0 : shift + 8;
                    }
                    done += n;
                }
            }
        }
        if (final ? last != 0 : b.real_bits_left() == 0) break;
    }
    if (final && (b.real_bits_left() >> 3) > 0) b.status |= kLeftover;
    if (q < out_end) b.status |= kShort;
    return b.status;
}

// The inverse of one filtered byte: p3d_video.h's FILTER rule read backwards.  x the residual, a / b / c the reconstructed bytes to the left, above and
// above-left.
P3D_PNG_HD int unfilter_byte(int type, int x, int a, int b, int c)
{
    int pred = 0;
    if (type == 1) pred = a;
    else if (type == 2) pred = b;
    else if (type == 3) pred = (a + b) >> 1;
    else if (type == 4) {
        const int p = a + b - c, pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
        pred = pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
    }
    return (x + pred) & 255;
}

} // namespace png
} // namespace p3d
#endif
