// Entropy decoding of baseline JPEG scans (p3d_video.h, "the way back from a file"; pix2pix3d_amd/video/jpeg_read.py).
//
// p3d_video_jpeg_unscan  a lane owns one restart interval: Huffman decoding is a chain of data-dependent shifts, so the parallel unit is the interval,
//                        which is byte-aligned, starts with predictors 0 and shares no bit with its neighbours.  The routine is jpeg_entropy.h, the text
//                        a host program runs under the sanitizers.  A work-group of one wave serves 64 intervals of ONE frame, whose four decode tables
//                        (5632 bytes) it copies into LDS first.  The coefficients are zeroed by one asynchronous fill before the launch, and a lane
//                        stores its non-zero values only: a handful of 2-byte stores per block instead of 128 scattered bytes.
#include "../p3d_common.h"
#include "p3d_video.h"
#include "jpeg_entropy.h"

namespace {

using namespace p3d;

static_assert(jpeg::kLookupBits == P3D_VIDEO_JPEG_LOOKUP_BITS && jpeg::kTableWords == P3D_VIDEO_JPEG_TABLE_WORDS, "jpeg_entropy.h and p3d_video.h agree");
static_assert(jpeg::kNoCode == P3D_VIDEO_JPEG_STATUS_NO_CODE && jpeg::kRun == P3D_VIDEO_JPEG_STATUS_RUN && jpeg::kSize == P3D_VIDEO_JPEG_STATUS_SIZE &&
              jpeg::kExhausted == P3D_VIDEO_JPEG_STATUS_EXHAUSTED && jpeg::kLeftover == P3D_VIDEO_JPEG_STATUS_LEFTOVER, "jpeg_entropy.h and p3d_video.h agree");
constexpr int kSetWords = 4 * jpeg::kTableWords;

struct UnscanArgs {
    const uint8_t* data; int64_t data_bytes;
    const int64_t* ranges;
    const uint32_t* tables; int n_sets;
    const int32_t* table_of_frame;
    int n_mcu, bpm, coded, restart, n_intervals, groups;      // groups: work-groups a frame
    int16_t* coefficients; int32_t* status;
};

__global__ void __launch_bounds__(kWave) jpeg_unscan_kernel(const UnscanArgs a)
{
    __shared__ uint32_t tables[kSetWords];
    const int lane = threadIdx.x;
    const int64_t f = blockIdx.x / (unsigned)a.groups;
    const int interval = (int)(blockIdx.x - f * a.groups) * kWave + lane;
    const int set = min(max(a.table_of_frame[f], 0), a.n_sets - 1);
    for (int i = lane; i < kSetWords; i += kWave) tables[i] = a.tables[(int64_t)set * kSetWords + i];
    __syncthreads();
    if (interval >= a.n_intervals) return;
    const int64_t slot = f * a.n_intervals + interval;
    const int64_t begin = min(max(a.ranges[2 * slot], (int64_t)0), a.data_bytes);
    const int64_t end = min(max(a.ranges[2 * slot + 1], begin), a.data_bytes);
    const int mcu0 = interval * a.restart;                                     // < n_mcu: n_intervals = ceil(n_mcu / restart)
    const int n_mcus = min(a.restart, a.n_mcu - mcu0);
    const int64_t frame_blocks = (int64_t)a.n_mcu * a.bpm;
    a.status[slot] = jpeg::unscan_interval(a.data, begin, end, tables, a.bpm, a.coded, mcu0, n_mcus, frame_blocks, a.coefficients + f * frame_blocks * 64);
}

} // namespace

extern "C" int p3d_video_jpeg_unscan(const uint8_t* data, int64_t data_bytes, const int64_t* ranges, const uint32_t* tables, int32_t n_sets,
                                     const int32_t* table_of_frame, int32_t n_frames, int32_t h, int32_t w, int32_t subsampling, int32_t components,
                                     int32_t restart, int16_t* coefficients, int32_t* status, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(n_frames >= 0 && h >= 0 && w >= 0, "video_jpeg_unscan: n_frames, h and w must be >= 0 (got %d, %d, %d)", n_frames, h, w);
    P3D_REQUIRE(subsampling == 0 || subsampling == 1, "video_jpeg_unscan: subsampling is 0 (4:4:4) or 1 (4:2:0) (got %d)", subsampling);
    P3D_REQUIRE(components == 3 || (components == 1 && subsampling == 0), "video_jpeg_unscan: components is 3, or 1 at subsampling 0 (got %d at %d)", components,
                subsampling);
    const int64_t hw = (int64_t)h * w;
    P3D_REQUIRE(hw < (1ll << 31) && hw * n_frames < (1ll << 31), "video_jpeg_unscan: %d x %d x %d pixels reach 2^31", n_frames, h, w);
    P3D_REQUIRE(data_bytes >= 0 && n_sets >= 1 && restart >= 1, "video_jpeg_unscan: data_bytes >= 0, n_sets >= 1 and restart >= 1 (got %lld, %d, %d)",
                (long long)data_bytes, n_sets, restart);
    if (hw * n_frames == 0) return P3D_OK;
    P3D_REQUIRE((data || data_bytes == 0) && ranges && tables && table_of_frame && coefficients && status,
                "video_jpeg_unscan: data, ranges, tables, table_of_frame, coefficients and status must be non-null");
    P3D_REQUIRE(((uintptr_t)ranges & 7u) == 0 && ((uintptr_t)tables & 3u) == 0 && ((uintptr_t)table_of_frame & 3u) == 0 && ((uintptr_t)coefficients & 1u) == 0 &&
                ((uintptr_t)status & 3u) == 0, "video_jpeg_unscan: ranges must be 8-byte aligned, tables, table_of_frame and status 4-byte, coefficients 2-byte");
    UnscanArgs a;
    const int mcu = 8 << subsampling;
    const int64_t n_mcu = (((int64_t)w + mcu - 1) / mcu) * (((int64_t)h + mcu - 1) / mcu);
    a.n_mcu = (int)n_mcu; a.bpm = subsampling ? 6 : 3; a.coded = components == 1 ? 1 : a.bpm;
    a.restart = (int)std::min<int64_t>(restart, n_mcu);                        // (an interval holds no more than the frame: interval * restart stays in int)
    a.n_intervals = (int)((n_mcu + a.restart - 1) / a.restart);
    a.groups = (a.n_intervals + kWave - 1) / kWave;
    const int64_t groups = (int64_t)n_frames * a.groups;
    P3D_REQUIRE(groups < (1ll << 31), "video_jpeg_unscan: %lld work-groups are too many for one launch", (long long)groups);
    a.data = data; a.data_bytes = data_bytes; a.ranges = ranges; a.tables = tables; a.n_sets = n_sets; a.table_of_frame = table_of_frame;
    a.coefficients = coefficients; a.status = status;
    const hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(coefficients, 0, sizeof(int16_t) * (size_t)n_frames * (size_t)n_mcu * a.bpm * 64, s) != hipSuccess)
        return fail(P3D_ERR_LAUNCH, "video_jpeg_unscan: memset failed");
    count_launch(FAM_AUX);
    hipLaunchKernelGGL(jpeg_unscan_kernel, dim3((unsigned)groups), dim3(kWave), 0, s, a);
    count_launch(FAM_AUX);
    return check_launch("video_jpeg_unscan");
}
