// Region tools on the uint8 label map of an edit session (p3d_regions.h; pix2pix3d_amd/regions.py).  Integer rules
// throughout: every result byte is defined by the header, and the torch formulations of regions.py produce the same bytes.
//
// p3d_label_components   union-find in the protocol of csrc/union_find.h, three launches.  init: a wave owns 64 consecutive pixels of one
//                        row and points every pixel at the first pixel of its run of equal labels inside those 64 (one ballot), so runs
//                        start out flat.  hook: one thread per pixel joins it to the left neighbour across a 64-pixel boundary, to the
//                        upper neighbour unless the pixel to the left makes the same join (both left pixels carry the label), and for
//                        connectivity 8 to a diagonal neighbour only where no 4-path through the 2 x 2 block already joins the two.
//                        flatten: every pixel reads its root.  The root of a finished tree is the smallest index of its component.
// p3d_label_nearest      pass 1, a work-group per strip of 64 columns: every lane builds, for its column and 64 rows at a time, a 64-bit word
//                        of site bits from 64 independent loads (a wave reads 64 consecutive bytes of a row); the words of the whole column
//                        stay in LDS, two waves carry the last site row above / the first below every 64-row chunk through them, and the nearest
//                        site row of a pixel is then two bit scans (clz / ctz) — no walk along the column.  pass 2, a work-group per 256
//                        pixels of a row with the row of pass-1 results in LDS: a lane visits the columns x - k, x + k for growing k
//                        (consecutive lanes read consecutive entries) and stops once k^2 exceeds its best d^2.
// p3d_label_warp         one launch; the four-pixel groups and the dword stores of paint_strokes_kernel (csrc/edit_ops.hip).  A source pixel
//                        outside the image re-reads a clamped one and the value is dropped: no load sits under a per-lane branch.
#include "../p3d_common.h"
#include "../union_find.h"
#include "p3d_regions.h"

namespace {

using namespace p3d;

// ---- components ----------------------------------------------------------------------------------------------------------------
constexpr int kRowsPerBlock = 4;                    // 256 threads = 4 waves = 4 rows of 64 pixels

struct CompArgs { const uint8_t* mask; int64_t pitch; int32_t* ids; int H, W, diagonals; };

__global__ void __launch_bounds__(256) components_init_kernel(const CompArgs a)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int x0 = blockIdx.x * kWave, x = x0 + lane, y = blockIdx.y * kRowsPerBlock + threadIdx.x / kWave;
    const int xc = min(x, a.W - 1), yc = min(y, a.H - 1);
    const uint8_t* row = a.mask + (int64_t)yc * a.pitch;
    const bool start = lane == 0 || row[xc] != row[max(xc - 1, 0)];
    const unsigned long long starts = __ballot(start) & ((2ull << lane) - 1ull);      // run starts at or before this lane; bit 0 is always set
    const int first = 63 - __clzll(starts);
    if (x < a.W && y < a.H) a.ids[(int64_t)y * a.W + x] = y * a.W + x0 + first;
}

__global__ void __launch_bounds__(256) components_hook_kernel(const CompArgs a)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int x = blockIdx.x * kWave + lane, y = blockIdx.y * kRowsPerBlock + threadIdx.x / kWave;
    if (x >= a.W || y >= a.H) return;
    const int xl = max(x - 1, 0), xr = min(x + 1, a.W - 1);
    const uint8_t* row = a.mask + (int64_t)y * a.pitch;
    const uint8_t* above = a.mask + (int64_t)max(y - 1, 0) * a.pitch;
    const int lab = row[x];
    const bool left = x > 0 && row[xl] == lab, up = y > 0 && above[x] == lab;
    const bool up_left = x > 0 && y > 0 && above[xl] == lab, up_right = x < a.W - 1 && y > 0 && above[xr] == lab;
    const int p = y * a.W + x;
    if (left && lane == 0) uf_union(a.ids, p, p - 1);                         // inside a wave's 64 pixels the init pass joined the run
    if (up && !(left && up_left)) uf_union(a.ids, p, p - a.W);                // else the pixel to the left joins the two rows
    if (a.diagonals) {
        if (up_left && !up && !left) uf_union(a.ids, p, p - a.W - 1);
        if (up_right && !up) uf_union(a.ids, p, p - a.W + 1);
    }
}

__global__ void __launch_bounds__(256) components_flatten_kernel(int32_t* ids, int32_t n)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    int32_t cur = uf_load(ids + v), next;
    while (cur > (next = uf_load(ids + cur))) cur = next;
    uf_store(ids + v, cur);                                                   // readers that race with this see the old parent or the root: both ancestors
}

// ---- nearest site --------------------------------------------------------------------------------------------------------------------
constexpr int kColumnWaves = 8;                     // pass 1: 512 threads, a wave per 64-row chunk of the strip at a time
constexpr int kNoRow = 0x7fff;                      // "no site below" in the int16 carries (rows are < 4096)

struct NearArgs {
    const uint8_t* mask; int64_t pitch;
    int32_t* rows;                                  // [H][W] workspace: nearest site row within the column, -1 for none
    int32_t* out;
    unsigned sites[8];
    int H, W, radius, chunks;
};

__global__ void __launch_bounds__(64 * kColumnWaves) nearest_columns_kernel(const NearArgs a)
{
    extern __shared__ __align__(16) unsigned char lds[];
    unsigned long long* const words = (unsigned long long*)lds;               // [chunks][64]: bit i of words[j][c] = pixel (64 j + i, c) is a site
    short* const above = (short*)(words + a.chunks * kWave);                  // [chunks][64]: the last site row in the chunks before j, or -1
    short* const below = above + a.chunks * kWave;                            // [chunks][64]: the first site row in the chunks after j, or kNoRow
    unsigned* const set = (unsigned*)(below + a.chunks * kWave);              // the 256 site bits

    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int x = blockIdx.x * kWave + lane, xc = min(x, a.W - 1);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) set[k] = a.sites[k];
    }
    __syncthreads();
    for (int j = wave; j < a.chunks; j += kColumnWaves) {
        unsigned long long word = 0;
#pragma unroll 16
        for (int i = 0; i < 64; ++i) {
            const int y = j * 64 + i;
            const unsigned lab = a.mask[(int64_t)min(y, a.H - 1) * a.pitch + xc];      // rows past the mask re-read the last row and are dropped
            const unsigned long long site = y < a.H ? (set[lab >> 5] >> (lab & 31)) & 1u : 0u;
            word |= site << i;
        }
        words[j * kWave + lane] = word;
    }
    __syncthreads();
    if (wave == 0) {
        int carry = -1;
        for (int j = 0; j < a.chunks; ++j) {
            above[j * kWave + lane] = (short)carry;
            const unsigned long long word = words[j * kWave + lane];
            carry = word ? j * 64 + 63 - __clzll(word) : carry;
        }
    } else if (wave == 1) {
        int carry = kNoRow;
        for (int j = a.chunks - 1; j >= 0; --j) {
            below[j * kWave + lane] = (short)carry;
            const unsigned long long word = words[j * kWave + lane];
            carry = word ? j * 64 + __ffsll(word) - 1 : carry;
        }
    }
    __syncthreads();
    if (x >= a.W) return;
    for (int j = wave; j < a.chunks; j += kColumnWaves) {
        const unsigned long long word = words[j * kWave + lane];
        const int ab = above[j * kWave + lane], be = below[j * kWave + lane];
        const int rows = min(64, a.H - j * 64);
        for (int i = 0; i < rows; ++i) {
            const int y = j * 64 + i;
            const unsigned long long at_or_above = word & ((2ull << i) - 1ull), under = i == 63 ? 0ull : word >> (i + 1);
            const int up = at_or_above ? j * 64 + 63 - __clzll(at_or_above) : ab;
            const int down = under ? y + __ffsll(under) : be;
            int row = -1;
            if (up >= 0 && down != kNoRow) row = y - up <= down - y ? up : down;       // the upper one on a tie
            else if (up >= 0) row = up;
            else if (down != kNoRow) row = down;
            a.rows[(int64_t)y * a.W + x] = row;                                          // a wave stores 256 consecutive bytes
        }
    }
}

__global__ void __launch_bounds__(256) nearest_rows_kernel(const NearArgs a)
{
    extern __shared__ __align__(16) unsigned char lds[];
    int* const row = (int*)lds;                                                // [W] <= 16 KB: pass 1's answers for this row
    const int y = blockIdx.y;
    const int32_t* const src = a.rows + (int64_t)y * a.W;
    for (int i = threadIdx.x; i < a.W; i += 256) row[i] = src[i];
    __syncthreads();
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= a.W) return;
    constexpr long long kNone = 0x7fffffffffffffffll;
    long long best = kNone;                                                    // (d^2 << 24) | index: d^2 < 2^25, index < 2^24
    const int kmax = a.radius < 0 ? a.W - 1 : min(a.radius, a.W - 1);
    for (int k = 0; k <= kmax && (long long)k * k <= (best >> 24); ++k) {
        const int xl = x - k, xr = x + k;
        const int sl = row[max(xl, 0)], sr = row[min(xr, a.W - 1)];
        const long long dl = y - sl, dr = y - sr, kk = (long long)k * k;
        const long long key_l = ((kk + dl * dl) << 24) | (long long)(sl * a.W + xl);
        const long long key_r = ((kk + dr * dr) << 24) | (long long)(sr * a.W + xr);
        best = (xl >= 0 && sl >= 0 && key_l < best) ? key_l : best;
        best = (xr < a.W && sr >= 0 && key_r < best) ? key_r : best;
    }
    const long long d2 = best >> 24;
    const bool found = best != kNone && (a.radius < 0 || d2 <= (long long)a.radius * a.radius);
    a.out[(int64_t)y * a.W + x] = found ? (int)(best & 0xffffff) : -1;
}

// ---- warp ----------------------------------------------------------------------------------------------------------------------
constexpr int kTileRows = 16, kTileGroups = 16;

struct WarpArgs {
    const uint8_t* mask; int64_t mask_pitch;
    const uint8_t* region; int64_t region_pitch;
    const uint8_t* under; int64_t under_pitch;
    uint8_t* dst; int64_t dst_pitch;
    long long c[6];
    int H, W, groups;
};

__global__ void __launch_bounds__(256) label_warp_kernel(const WarpArgs a)
{
    const int tid = threadIdx.x;
    const int g = blockIdx.x * kTileGroups + (tid % kTileGroups);
    const int y = blockIdx.y * kTileRows + tid / kTileGroups;
    const int yc = min(y, a.H - 1);                                 // rows past the mask re-read the last row and store nothing
    uint8_t* const drow = a.dst + (int64_t)yc * a.dst_pitch;
    const int head = (int)((4 - (((uintptr_t)drow) & 3u)) & 3u);    // pixels in front of the row's first 4-byte boundary
    const int x0 = g == 0 ? 0 : head + 4 * (g - 1);
    const int x1 = g == 0 ? min(head, a.W) : min(a.W, x0 + 4);
    const int cnt = (y < a.H && g < a.groups) ? max(x1 - x0, 0) : 0;
    const int xb = min(x0, a.W - 1);

    const uint8_t* const urow = a.under + (int64_t)yc * a.under_pitch;
    const long long bx = a.c[1] * yc + a.c[2] + 32768, by = a.c[4] * yc + a.c[5] + 32768;
    unsigned lab[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int px = min(xb + i, a.W - 1);
        const long long qx = (a.c[0] * px + bx) >> 16, qy = (a.c[3] * px + by) >> 16;
        const bool inside = qx >= 0 && qx < a.W && qy >= 0 && qy < a.H;
        const int sx = (int)min(max(qx, 0ll), (long long)a.W - 1), sy = (int)min(max(qy, 0ll), (long long)a.H - 1);
        const unsigned m = a.mask[(int64_t)sy * a.mask_pitch + sx], r = a.region[(int64_t)sy * a.region_pitch + sx], u = urow[px];
        lab[i] = (inside && r != 0) ? m : u;
    }

    uint8_t* const dp = drow + xb;
    if (cnt == 4 && g > 0) {
        *(unsigned*)dp = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < cnt) dp[i] = (uint8_t)lab[i];
    }
}

bool mask_size_ok(int32_t h, int32_t w) { return h >= 1 && w >= 1 && h <= P3D_PAINT_MAX_SIZE && w <= P3D_PAINT_MAX_SIZE; }

} // namespace

extern "C" int p3d_label_components(const uint8_t* mask, int64_t mask_row_pitch, int32_t* ids, int32_t h, int32_t w, int32_t connectivity,
                                    p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(mask && ids, "label_components: mask and ids must be non-null");
    P3D_REQUIRE(mask_size_ok(h, w), "label_components: the mask is 1 .. %d pixels a side (got %d x %d)", P3D_PAINT_MAX_SIZE, h, w);
    P3D_REQUIRE(connectivity == 4 || connectivity == 8, "label_components: connectivity is 4 or 8 (got %d)", connectivity);
    P3D_REQUIRE(mask_row_pitch >= w, "label_components: the row pitch is shorter than the row");
    P3D_REQUIRE(((uintptr_t)ids & 3u) == 0, "label_components: ids must be 4-byte aligned");
    CompArgs a;
    a.mask = mask; a.pitch = mask_row_pitch; a.ids = ids; a.H = h; a.W = w; a.diagonals = connectivity == 8;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(w, kWave), (unsigned)ceil_div(h, kRowsPerBlock));
    hipLaunchKernelGGL(components_init_kernel, grid, dim3(256), 0, s, a);
    count_launch(FAM_AUX);
    hipLaunchKernelGGL(components_hook_kernel, grid, dim3(256), 0, s, a);
    count_launch(FAM_AUX);
    hipLaunchKernelGGL(components_flatten_kernel, dim3((unsigned)ceil_div((int64_t)h * w, 256)), dim3(256), 0, s, ids, h * w);
    count_launch(FAM_AUX);
    return check_launch("label_components");
}

extern "C" int p3d_label_nearest(const uint8_t* mask, int64_t mask_row_pitch, const uint32_t sites[8], int32_t radius, int32_t* workspace,
                                 int32_t* nearest, int32_t h, int32_t w, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(mask && sites && workspace && nearest, "label_nearest: mask, sites, workspace and nearest must be non-null");
    P3D_REQUIRE(mask_size_ok(h, w), "label_nearest: the mask is 1 .. %d pixels a side (got %d x %d)", P3D_PAINT_MAX_SIZE, h, w);
    P3D_REQUIRE(mask_row_pitch >= w, "label_nearest: the row pitch is shorter than the row");
    P3D_REQUIRE(workspace != nearest, "label_nearest: the workspace must not be the result");
    P3D_REQUIRE((((uintptr_t)workspace | (uintptr_t)nearest) & 3u) == 0, "label_nearest: workspace and nearest must be 4-byte aligned");
    NearArgs a;
    a.mask = mask; a.pitch = mask_row_pitch; a.rows = workspace; a.out = nearest; a.H = h; a.W = w;
    a.radius = radius < 0 ? -1 : (radius > 2 * P3D_PAINT_MAX_SIZE ? 2 * P3D_PAINT_MAX_SIZE : radius);      // past the diagonal every radius is the same
    a.chunks = ceil_div(h, 64);
    for (int k = 0; k < 8; ++k) a.sites[k] = sites[k];
    const hipStream_t s = (hipStream_t)stream;
    const size_t lds_columns = (size_t)a.chunks * kWave * (sizeof(unsigned long long) + 2 * sizeof(short)) + 8 * sizeof(unsigned);      // <= 48 KB + 32
    hipLaunchKernelGGL(nearest_columns_kernel, dim3((unsigned)ceil_div(w, kWave)), dim3(64 * kColumnWaves), lds_columns, s, a);
    count_launch(FAM_AUX);
    hipLaunchKernelGGL(nearest_rows_kernel, dim3((unsigned)ceil_div(w, 256), (unsigned)h), dim3(256), (size_t)w * sizeof(int), s, a);
    count_launch(FAM_AUX);
    return check_launch("label_nearest");
}

extern "C" int p3d_label_warp(const uint8_t* mask, int64_t mask_row_pitch, const uint8_t* region, int64_t region_row_pitch, const uint8_t* under,
                              int64_t under_row_pitch, uint8_t* dst, int64_t dst_row_pitch, const int64_t coef[6], int32_t h, int32_t w,
                              p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(mask && region && under && dst && coef, "label_warp: mask, region, under, dst and coef must be non-null");
    P3D_REQUIRE(mask_size_ok(h, w), "label_warp: the mask is 1 .. %d pixels a side (got %d x %d)", P3D_PAINT_MAX_SIZE, h, w);
    P3D_REQUIRE(mask_row_pitch >= w && region_row_pitch >= w && under_row_pitch >= w && dst_row_pitch >= w, "label_warp: a row pitch is shorter than the row");
    P3D_REQUIRE(dst != mask && dst != region && dst != under, "label_warp: the mask is written out of place");
    WarpArgs a;
    for (int k = 0; k < 6; ++k) {
        const int log2_bound = (k == 2 || k == 5) ? P3D_LABEL_MAX_TRANSLATION_LOG2 : P3D_LABEL_MAX_LINEAR_LOG2;
        P3D_REQUIRE(coef[k] >= -(1ll << log2_bound) && coef[k] <= (1ll << log2_bound), "label_warp: coef[%d] = %lld leaves +-2^%d", k, (long long)coef[k], log2_bound);
        a.c[k] = coef[k];
    }
    a.mask = mask; a.mask_pitch = mask_row_pitch; a.region = region; a.region_pitch = region_row_pitch; a.under = under; a.under_pitch = under_row_pitch;
    a.dst = dst; a.dst_pitch = dst_row_pitch; a.H = h; a.W = w; a.groups = (w + 3) / 4 + 1;
    const dim3 grid((unsigned)ceil_div(a.groups, kTileGroups), (unsigned)ceil_div(h, kTileRows));
    hipLaunchKernelGGL(label_warp_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    count_launch(FAM_AUX);
    return check_launch("label_warp");
}
