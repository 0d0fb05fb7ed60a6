// The entropy decoder of pix2pix3d_amd/csrc/video/jpeg_entropy.h on the host, interval after interval: the text the device runs a lane of, built with
// any C++14 compiler and no HIP — in particular with the address and undefined-behaviour sanitizers, which is what tests/test_video_jpeg_read_host.py does:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I pix2pix3d_amd/csrc/video tools/jpeg_unscan_check.cpp -o check
//     ./check cases.bin results.bin
//
// cases.bin (little endian, written by tests/jpeg_read_cases.py): int32 magic 'J','U','C','1', int32 n_cases; per case int32 h, w, subsampling, components,
// restart, n_frames, n_sets, int64 data_bytes, then ranges int64 [n_frames][n_intervals][2], tables uint32 [n_sets][4][352], table_of_frame int32
// [n_frames] and the data bytes.  results.bin: per case coefficients int16 [n_frames][n_mcu][bpm][64], then status int32 [n_frames][n_intervals].
// Every buffer is a heap block of exactly its size, so a read or a store one byte out of place is a sanitizer report.  Exit status 0: all cases ran.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "jpeg_entropy.h"

namespace {

template <class T> bool read(std::FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

template <class T> bool read(std::FILE* f, T& v) { return std::fread(&v, sizeof(T), 1, f) == 1; }

int fail(const char* what, int c)
{
    std::fprintf(stderr, "jpeg_unscan_check: case %d: %s\n", c, what);
    return 1;
}

} // namespace

int main(int argc, char** argv)
{
    using namespace p3d::jpeg;
    if (argc != 3) { std::fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    std::FILE* const in = std::fopen(argv[1], "rb");
    std::FILE* const out = in ? std::fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { std::fprintf(stderr, "jpeg_unscan_check: cannot open %s\n", in ? argv[2] : argv[1]); return 2; }
    int32_t magic = 0, n_cases = 0;
    if (!read(in, magic) || !read(in, n_cases) || magic != 0x3143554A || n_cases < 0) return fail("not a case file", -1);
    for (int c = 0; c < n_cases; ++c) {
        int32_t head[7];
        int64_t data_bytes = 0;
        if (std::fread(head, sizeof(int32_t), 7, in) != 7 || !read(in, data_bytes)) return fail("the file ends inside a case", c);
        const int h = head[0], w = head[1], subsampling = head[2], components = head[3], n_frames = head[5], n_sets = head[6];
        if (h < 1 || w < 1 || h > 65535 || w > 65535 || (subsampling != 0 && subsampling != 1) || (components != 3 && !(components == 1 && subsampling == 0)) ||
            head[4] < 1 || n_frames < 1 || n_frames > 4096 || n_sets < 1 || n_sets > 4096 || data_bytes < 0 || data_bytes > (1ll << 30))
            return fail("arguments out of range", c);
        // the geometry, as p3d_video_jpeg_unscan derives it
        const int mcu = 8 << subsampling, bpm = subsampling ? 6 : 3, coded = components == 1 ? 1 : bpm;
        const int64_t n_mcu = (int64_t)((w + mcu - 1) / mcu) * ((h + mcu - 1) / mcu);
        const int restart = (int)std::min<int64_t>(head[4], n_mcu);
        const int n_intervals = (int)((n_mcu + restart - 1) / restart);
        std::vector<int64_t> ranges;
        std::vector<uint32_t> tables;
        std::vector<int32_t> table_of_frame;
        std::vector<uint8_t> data;
        if (!read(in, ranges, (size_t)n_frames * n_intervals * 2) || !read(in, tables, (size_t)n_sets * 4 * kTableWords) ||
            !read(in, table_of_frame, (size_t)n_frames) || !read(in, data, (size_t)data_bytes))
            return fail("the file ends inside a case", c);
        const int64_t frame_blocks = n_mcu * bpm;
        std::vector<int16_t> coefficients((size_t)n_frames * frame_blocks * 64, 0);      // the fill
        std::vector<int32_t> status((size_t)n_frames * n_intervals, 0);
        for (int f = 0; f < n_frames; ++f) {
            const int set = std::min(std::max(table_of_frame[f], 0), n_sets - 1);
            for (int i = 0; i < n_intervals; ++i) {                                     // what a lane does
                const int64_t slot = (int64_t)f * n_intervals + i;
                const int64_t begin = std::min(std::max<int64_t>(ranges[2 * slot], 0), data_bytes);
                const int64_t end = std::min(std::max(ranges[2 * slot + 1], begin), data_bytes);
                const int mcu0 = i * restart;
                const int n_mcus = (int)std::min<int64_t>(restart, n_mcu - mcu0);
                status[slot] = unscan_interval(data.data(), begin, end, tables.data() + (size_t)set * 4 * kTableWords, bpm, coded, mcu0, n_mcus, frame_blocks,
                                               coefficients.data() + (size_t)f * frame_blocks * 64);
            }
        }
        if (std::fwrite(coefficients.data(), sizeof(int16_t), coefficients.size(), out) != coefficients.size() ||
            std::fwrite(status.data(), sizeof(int32_t), status.size(), out) != status.size())
            return fail("cannot write the results", c);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return fail("cannot write the results", n_cases);
    std::printf("jpeg_unscan_check: %d cases\n", n_cases);
    return 0;
}
