// The inflate routine of pix2pix3d_amd/csrc/video/png_inflate.h on the host, part after part: the text the device runs a lane of, built with any C++14
// compiler and no HIP — in particular with the address and undefined-behaviour sanitizers, which is what tests/test_video_png_read_host.py does:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I pix2pix3d_amd/csrc/video tools/png_inflate_check.cpp -o check
//     ./check cases.bin results.bin
//
// cases.bin (little endian, written by tests/png_read_cases.py): int32 magic 'P','I','C','1', int32 n_cases; per case int64 data_bytes, int64 out_bytes,
// int64 n_parts, then parts int64 [n_parts][5] (in_begin, in_end, out_begin, out_end, final) and the data bytes.  results.bin: per case the output
// uint8 [out_bytes], then status int32 [n_parts].  Every buffer is a heap block of exactly its size — the decode state of a part included —, so a read
// or a store one byte out of place is a sanitizer report.  Exit status 0: all cases ran.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "png_inflate.h"

namespace {

template <class T> bool read(std::FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

template <class T> bool read(std::FILE* f, T& v) { return std::fread(&v, sizeof(T), 1, f) == 1; }

int fail(const char* what, int c)
{
    std::fprintf(stderr, "png_inflate_check: case %d: %s\n", c, what);
    return 1;
}

int64_t clamp(int64_t v, int64_t lo, int64_t hi) { return std::min(std::max(v, lo), hi); }

} // namespace

int main(int argc, char** argv)
{
    using namespace p3d::png;
    if (argc != 3) { std::fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    std::FILE* const in = std::fopen(argv[1], "rb");
    std::FILE* const out_file = in ? std::fopen(argv[2], "wb") : nullptr;
    if (!in || !out_file) { std::fprintf(stderr, "png_inflate_check: cannot open %s\n", in ? argv[2] : argv[1]); return 2; }
    int32_t magic = 0, n_cases = 0;
    if (!read(in, magic) || !read(in, n_cases) || magic != 0x31434950 || n_cases < 0) return fail("not a case file", -1);
    for (int c = 0; c < n_cases; ++c) {
        int64_t data_bytes = 0, out_bytes = 0, n_parts = 0;
        if (!read(in, data_bytes) || !read(in, out_bytes) || !read(in, n_parts)) return fail("the file ends inside a case", c);
        if (data_bytes < 0 || data_bytes > (1ll << 30) || out_bytes < 0 || out_bytes > (1ll << 30) || n_parts < 0 || n_parts > (1 << 20))
            return fail("arguments out of range", c);
        std::vector<int64_t> parts;
        std::vector<uint8_t> data;
        if (!read(in, parts, (size_t)n_parts * 5) || !read(in, data, (size_t)data_bytes)) return fail("the file ends inside a case", c);
        std::vector<uint8_t> out((size_t)out_bytes, 0);                                 // the fill
        std::vector<int32_t> status((size_t)n_parts, 0);
        for (int64_t i = 0; i < n_parts; ++i) {                                         // what a lane does
            const int64_t* const p = parts.data() + 5 * i;
            const int64_t in_begin = clamp(p[0], 0, data_bytes), in_end = clamp(p[1], in_begin, data_bytes);
            const int64_t out_begin = clamp(p[2], 0, out_bytes), out_end = clamp(p[3], out_begin, out_bytes);
            std::vector<uint16_t> words(kStateHalves, 0);
            const State s = {words.data(), 1};
            status[(size_t)i] = inflate_part(data.data(), in_begin, in_end, out.data(), out_begin, out_end, p[4] != 0, s);
        }
        if (std::fwrite(out.data(), 1, out.size(), out_file) != out.size() ||
            std::fwrite(status.data(), sizeof(int32_t), status.size(), out_file) != status.size())
            return fail("cannot write the results", c);
    }
    std::fclose(in);
    if (std::fclose(out_file) != 0) return fail("cannot write the results", n_cases);
    std::printf("png_inflate_check: %d cases\n", n_cases);
    return 0;
}
