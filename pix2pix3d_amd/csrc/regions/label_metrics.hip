// Agreement metrics on uint8 label maps (p3d_regions.h; pix2pix3d_amd/evaluate.py).  Integer rules throughout: the three
// counters accumulate with 64-bit integer atomics, so every sum is independent of the order the hardware takes the pixels in, and the torch
// formulations of evaluate.py produce the same bytes.
//
// p3d_label_confusion            one launch.  The maps are cut into rows (a frame's rows; one row per frame where the rows of every operand
//                                lie back to back; ONE row where the frames do too) and a row into items of 16 pixels: item 0 is the scalar head
//                                in front of the truth row's first 16-byte boundary, the others one 16-byte load per operand where the operands'
//                                rows share the truth row's alignment and byte loads where they do not (and in the tail).  A lane turns its item
//                                into 16 keys t * n + p (n * n: left out; -1: past the row) in registers.  Label maps are large uniform regions,
//                                so a wave first votes: when all 1024 keys equal the first lane's, lane 0 adds 1024 once.  Otherwise a lane
//                                collapses runs of equal keys and adds one count per run.  The counters are a private uint32 matrix per WAVE in
//                                LDS (n * n + 1 <= 1025 words, 4 waves: 16.4 KB a work-group), folded once per work-group: 64-bit global atomic
//                                adds of the non-zero cells only.  At most kConfGrid work-groups walk the tiles of 256 items.
// p3d_label_boundary             one launch; the four-pixel groups and the dword stores of label_warp_kernel.  A neighbour outside the image
//                                re-reads the pixel itself, which never differs.
// p3d_label_distance_histogram   one launch; a uint32 histogram of bins + 2 slots per work-group in LDS.  The three slots many pixels share (d2 = 0,
//                                saturated, no site) are counted by a ballot and added by one lane; the others by LDS atomics.  One fold per
//                                work-group, non-zero slots only.
#include "../p3d_common.h"
#include "p3d_regions.h"

namespace {

using namespace p3d;

constexpr int kMaxLabels = P3D_LABEL_MAX_LABELS, kMaxBins = P3D_LABEL_MAX_BINS, kMaxFrames = P3D_LABEL_MAX_FRAMES;

// ---- confusion ---------------------------------------------------------------------------------------------------------------------
constexpr int kConfWaves = 4, kItem = 16, kTileItems = kWave * kConfWaves;
constexpr int kConfGrid = 2048;                     // 8 work-groups a CU; a wave then counts < 2^28 pixels into a uint32 cell at the largest call

struct ConfArgs {
    const uint8_t* truth; int64_t t_row, t_frame;
    const uint8_t* pred;  int64_t p_row, p_frame;
    const uint8_t* valid; int64_t v_row, v_frame;
    unsigned long long* counts;
    int64_t width, tiles, tiles_per_row;            // pixels of a row; tiles = rows * tiles_per_row
    int rows_per_frame, n;
};

__device__ __forceinline__ unsigned byte_of(const uint4& v, int i)
{
    const unsigned word = i < 4 ? v.x : i < 8 ? v.y : i < 12 ? v.z : v.w;
    return (word >> ((i & 3) * 8)) & 0xffu;
}

__global__ void __launch_bounds__(kTileItems) label_confusion_kernel(const ConfArgs a)
{
    extern __shared__ __align__(16) unsigned char lds[];
    unsigned* const cells = (unsigned*)lds;                                    // [kConfWaves][n * n + 1]
    const int n_cells = a.n * a.n + 1, left_out = a.n * a.n;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    unsigned* const mine = cells + (tid / kWave) * n_cells;
    for (int c = tid; c < kConfWaves * n_cells; c += kTileItems) cells[c] = 0u;
    __syncthreads();

    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {       // uniform over the work-group: every lane reaches the vote
        const int64_t row = tile / a.tiles_per_row, item = (tile - row * a.tiles_per_row) * kTileItems + tid;
        const int64_t frame = row / a.rows_per_frame, y = row - frame * a.rows_per_frame;
        const uint8_t* const trow = a.truth + frame * a.t_frame + y * a.t_row;
        const uint8_t* const prow = a.pred + frame * a.p_frame + y * a.p_row;
        const uint8_t* const vrow = a.valid ? a.valid + frame * a.v_frame + y * a.v_row : nullptr;
        const int64_t head = min((int64_t)((16u - ((uintptr_t)trow & 15u)) & 15u), a.width);
        const int64_t x0 = item == 0 ? 0 : head + (item - 1) * kItem;
        const int64_t x1 = item == 0 ? head : min(a.width, x0 + kItem);
        const int cnt = (int)max(x1 - x0, (int64_t)0);                          // 0 for the items past the row's end
        const bool wide = cnt == kItem && item > 0 && (((uintptr_t)(prow + x0)) & 15u) == 0 && (!vrow || (((uintptr_t)(vrow + x0)) & 15u) == 0);

        int key[kItem];
        if (wide) {
            const uint4 t4 = *(const uint4*)(trow + x0), p4 = *(const uint4*)(prow + x0);
            uint4 v4 = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
            if (vrow) v4 = *(const uint4*)(vrow + x0);
#pragma unroll
            for (int i = 0; i < kItem; ++i) {
                const int t = (int)byte_of(t4, i), p = (int)byte_of(p4, i);
                key[i] = (t < a.n && p < a.n && byte_of(v4, i) != 0u) ? t * a.n + p : left_out;
            }
        } else {
#pragma unroll
            for (int i = 0; i < kItem; ++i) {
                key[i] = -1;
                if (i < cnt) {
                    const int t = trow[x0 + i], p = prow[x0 + i];
                    const bool ok = vrow ? vrow[x0 + i] != 0 : true;
                    key[i] = (t < a.n && p < a.n && ok) ? t * a.n + p : left_out;
                }
            }
        }

        bool same = true;
#pragma unroll
        for (int i = 1; i < kItem; ++i) same = same && key[i] == key[0];
        const int first = __builtin_amdgcn_readfirstlane(key[0]);
        if (__all(same && key[0] == first)) {                                  // the whole wave holds one key: one add
            if (lane == 0 && first >= 0) atomicAdd(mine + first, (unsigned)(kWave * kItem));
        } else {
            int cur = key[0], run = 1;
#pragma unroll
            for (int i = 1; i < kItem; ++i) {
                if (key[i] == cur) {
                    ++run;
                } else {
                    if (cur >= 0) atomicAdd(mine + cur, (unsigned)run);
                    cur = key[i];
                    run = 1;
                }
            }
            if (cur >= 0) atomicAdd(mine + cur, (unsigned)run);
        }
    }

    __syncthreads();
    for (int c = tid; c < n_cells; c += kTileItems) {
        unsigned long long sum = 0;
#pragma unroll
        for (int wv = 0; wv < kConfWaves; ++wv) sum += cells[wv * n_cells + c];
        if (sum) atomicAdd(a.counts + c, sum);
    }
}

// ---- boundary ----------------------------------------------------------------------------------------------------------------------
constexpr int kTileRows = 16, kTileGroups = 16;

struct BoundArgs { const uint8_t* mask; int64_t mask_pitch; uint8_t* out; int64_t out_pitch; int H, W, groups; };

__global__ void __launch_bounds__(256) label_boundary_kernel(const BoundArgs a)
{
    const int tid = threadIdx.x;
    const int g = blockIdx.x * kTileGroups + (tid % kTileGroups);
    const int y = blockIdx.y * kTileRows + tid / kTileGroups;
    const int yc = min(y, a.H - 1);                                 // rows past the mask re-read the last row and store nothing
    uint8_t* const orow = a.out + (int64_t)yc * a.out_pitch;
    const int head = (int)((4 - (((uintptr_t)orow) & 3u)) & 3u);    // pixels in front of the row's first 4-byte boundary
    const int x0 = g == 0 ? 0 : head + 4 * (g - 1);
    const int x1 = g == 0 ? min(head, a.W) : min(a.W, x0 + 4);
    const int cnt = (y < a.H && g < a.groups) ? max(x1 - x0, 0) : 0;
    const int xb = min(x0, a.W - 1);

    const uint8_t* const row = a.mask + (int64_t)yc * a.mask_pitch;
    const uint8_t* const above = a.mask + (int64_t)max(yc - 1, 0) * a.mask_pitch;
    const uint8_t* const below = a.mask + (int64_t)min(yc + 1, a.H - 1) * a.mask_pitch;
    unsigned lab[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int px = min(xb + i, a.W - 1);
        const unsigned c = row[px], l = row[max(px - 1, 0)], r = row[min(px + 1, a.W - 1)], u = above[px], d = below[px];
        lab[i] = (l != c || r != c || u != c || d != c) ? c : 255u;       // a neighbour outside the image is the pixel itself
    }

    uint8_t* const dp = orow + xb;
    if (cnt == 4 && g > 0) {
        *(unsigned*)dp = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < cnt) dp[i] = (uint8_t)lab[i];
    }
}

// ---- distance histogram ------------------------------------------------------------------------------------------------------------
constexpr int kHistGrid = 512;

struct HistArgs {
    const uint8_t* from; int64_t pitch;
    const int32_t* nearest;
    unsigned long long* hist;
    unsigned sites[8];
    int H, W, bins;
};

__global__ void __launch_bounds__(256) label_distance_histogram_kernel(const HistArgs a)
{
    extern __shared__ __align__(16) unsigned char lds[];
    unsigned* const slots = (unsigned*)lds;                                    // [bins + 2]
    unsigned* const set = slots + a.bins + 2;                                  // the 256 site bits
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    for (int c = tid; c < a.bins + 2; c += 256) slots[c] = 0u;
    if (tid < 8) set[tid] = a.sites[tid];
    __syncthreads();

    const int n = a.H * a.W;                                                   // <= 2^24
    for (int base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {     // uniform over the work-group: every lane reaches the ballots
        const int p = base + tid, pc = min(p, n - 1);
        const int py = pc / a.W, px = pc - py * a.W;
        const unsigned lab = a.from[(int64_t)py * a.pitch + px];
        const bool in = p < n && ((set[lab >> 5] >> (lab & 31)) & 1u) != 0u;
        const int q = a.nearest[pc];
        const int qy = max(q, 0) / a.W, qx = max(q, 0) - qy * a.W;
        const long long dx = px - qx, dy = py - qy, d2 = dx * dx + dy * dy;
        const int slot = q < 0 ? a.bins + 1 : (int)min(d2, (long long)a.bins);
        const unsigned long long at_zero = __ballot(in && slot == 0), beyond = __ballot(in && slot == a.bins), none = __ballot(in && slot == a.bins + 1);
        if (lane == 0) {
            if (at_zero) atomicAdd(slots, (unsigned)__popcll(at_zero));
            if (beyond) atomicAdd(slots + a.bins, (unsigned)__popcll(beyond));
            if (none) atomicAdd(slots + a.bins + 1, (unsigned)__popcll(none));
        }
        if (in && slot > 0 && slot < a.bins) atomicAdd(slots + slot, 1u);
    }

    __syncthreads();
    for (int c = tid; c < a.bins + 2; c += 256) {
        const unsigned v = slots[c];
        if (v) atomicAdd(a.hist + c, (unsigned long long)v);
    }
}

bool map_size_ok(int32_t h, int32_t w) { return h >= 1 && w >= 1 && h <= P3D_PAINT_MAX_SIZE && w <= P3D_PAINT_MAX_SIZE; }

} // namespace

extern "C" int p3d_label_confusion(const uint8_t* truth, int64_t truth_row_pitch, int64_t truth_frame_pitch, const uint8_t* pred,
                                   int64_t pred_row_pitch, int64_t pred_frame_pitch, const uint8_t* valid, int64_t valid_row_pitch,
                                   int64_t valid_frame_pitch, int32_t frames, int32_t h, int32_t w, int32_t n_labels, int64_t* counts,
                                   p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(n_labels >= 1 && n_labels <= kMaxLabels, "label_confusion: n_labels is 1 .. %d (got %d)", kMaxLabels, n_labels);
    P3D_REQUIRE(frames >= 0 && frames <= kMaxFrames, "label_confusion: frames is 0 .. %d (got %d)", kMaxFrames, frames);
    P3D_REQUIRE(map_size_ok(h, w), "label_confusion: a map is 1 .. %d pixels a side (got %d x %d)", P3D_PAINT_MAX_SIZE, h, w);
    if (frames == 0) return P3D_OK;
    P3D_REQUIRE(truth && pred && counts, "label_confusion: truth, pred and counts must be non-null");
    P3D_REQUIRE(truth_row_pitch >= w && pred_row_pitch >= w && (!valid || valid_row_pitch >= w), "label_confusion: a row pitch is shorter than the row");
    if (frames > 1) {
        const int64_t last = (int64_t)(h - 1);
        P3D_REQUIRE(truth_frame_pitch >= last * truth_row_pitch + w && pred_frame_pitch >= last * pred_row_pitch + w &&
                    (!valid || valid_frame_pitch >= last * valid_row_pitch + w), "label_confusion: a frame pitch is shorter than the frame");
    }
    P3D_REQUIRE(((uintptr_t)counts & 7u) == 0, "label_confusion: counts must be 8-byte aligned");

    ConfArgs a;
    a.truth = truth; a.t_row = truth_row_pitch; a.t_frame = frames > 1 ? truth_frame_pitch : 0;
    a.pred = pred; a.p_row = pred_row_pitch; a.p_frame = frames > 1 ? pred_frame_pitch : 0;
    a.valid = valid; a.v_row = valid ? valid_row_pitch : 0; a.v_frame = (valid && frames > 1) ? valid_frame_pitch : 0;
    a.counts = (unsigned long long*)counts; a.n = n_labels;
    const int64_t frame_pixels = (int64_t)h * w;
    const bool rows_abut = h == 1 || (truth_row_pitch == w && pred_row_pitch == w && (!valid || valid_row_pitch == w));
    const bool frames_abut = rows_abut && (frames == 1 || (truth_frame_pitch == frame_pixels && pred_frame_pitch == frame_pixels &&
                                                            (!valid || valid_frame_pitch == frame_pixels)));
    int64_t rows;
    if (frames_abut)    { rows = 1; a.rows_per_frame = 1; a.width = frame_pixels * frames; }      // one row: the frame pitches are not used (frame 0 only)
    else if (rows_abut) { rows = frames; a.rows_per_frame = 1; a.width = frame_pixels; }          // a row per frame: the row pitches are not used (y = 0 only)
    else                { rows = (int64_t)frames * h; a.rows_per_frame = h; a.width = w; }
    const int64_t items = (a.width + kItem - 1) / kItem + 1;                                      // the head item and the 16-pixel ones
    a.tiles_per_row = (items + kTileItems - 1) / kTileItems;
    a.tiles = rows * a.tiles_per_row;
    const unsigned grid = (unsigned)(a.tiles < kConfGrid ? a.tiles : kConfGrid);
    const size_t lds_bytes = (size_t)kConfWaves * (n_labels * n_labels + 1) * sizeof(unsigned);
    hipLaunchKernelGGL(label_confusion_kernel, dim3(grid), dim3(kTileItems), lds_bytes, (hipStream_t)stream, a);
    count_launch(FAM_AUX);
    return check_launch("label_confusion");
}

extern "C" int p3d_label_boundary(const uint8_t* mask, int64_t mask_row_pitch, uint8_t* out, int64_t out_row_pitch, int32_t h, int32_t w,
                                  p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(mask && out, "label_boundary: mask and out must be non-null");
    P3D_REQUIRE(map_size_ok(h, w), "label_boundary: the mask is 1 .. %d pixels a side (got %d x %d)", P3D_PAINT_MAX_SIZE, h, w);
    P3D_REQUIRE(mask_row_pitch >= w && out_row_pitch >= w, "label_boundary: a row pitch is shorter than the row");
    const uintptr_t m0 = (uintptr_t)mask, m1 = m0 + (uintptr_t)((int64_t)(h - 1) * mask_row_pitch + w);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)((int64_t)(h - 1) * out_row_pitch + w);
    P3D_REQUIRE(m1 <= o0 || o1 <= m0, "label_boundary: the map is written out of place (mask and out overlap)");
    BoundArgs a;
    a.mask = mask; a.mask_pitch = mask_row_pitch; a.out = out; a.out_pitch = out_row_pitch; a.H = h; a.W = w; a.groups = (w + 3) / 4 + 1;
    const dim3 grid((unsigned)ceil_div(a.groups, kTileGroups), (unsigned)ceil_div(h, kTileRows));
    hipLaunchKernelGGL(label_boundary_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    count_launch(FAM_AUX);
    return check_launch("label_boundary");
}

extern "C" int p3d_label_distance_histogram(const uint8_t* from, int64_t from_row_pitch, const uint32_t sites[8], const int32_t* nearest,
                                            int32_t bins, int64_t* hist, int32_t h, int32_t w, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(from && sites && nearest && hist, "label_distance_histogram: from, sites, nearest and hist must be non-null");
    P3D_REQUIRE(map_size_ok(h, w), "label_distance_histogram: the map is 1 .. %d pixels a side (got %d x %d)", P3D_PAINT_MAX_SIZE, h, w);
    P3D_REQUIRE(from_row_pitch >= w, "label_distance_histogram: the row pitch is shorter than the row");
    P3D_REQUIRE(bins >= 1 && bins <= kMaxBins, "label_distance_histogram: bins is 1 .. %d (got %d)", kMaxBins, bins);
    P3D_REQUIRE(((uintptr_t)nearest & 3u) == 0 && ((uintptr_t)hist & 7u) == 0, "label_distance_histogram: nearest must be 4-byte and hist 8-byte aligned");
    HistArgs a;
    a.from = from; a.pitch = from_row_pitch; a.nearest = nearest; a.hist = (unsigned long long*)hist; a.H = h; a.W = w; a.bins = bins;
    for (int k = 0; k < 8; ++k) a.sites[k] = sites[k];
    const int blocks = ceil_div((int64_t)h * w, 256);
    const size_t lds_bytes = (size_t)(bins + 2 + 8) * sizeof(unsigned);
    hipLaunchKernelGGL(label_distance_histogram_kernel, dim3((unsigned)(blocks < kHistGrid ? blocks : kHistGrid)), dim3(256), lds_bytes,
                       (hipStream_t)stream, a);
    count_launch(FAM_AUX);
    return check_launch("label_distance_histogram");
}
