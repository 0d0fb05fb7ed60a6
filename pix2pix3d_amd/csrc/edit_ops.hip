// The device pieces of an edit session (pix2pix3d_amd/edit.py), the compute core of the reference's applications/demo/qt_demo_seg2cat.py:
//
//   p3d_paint_strokes   every brush stroke of the session into the uint8 label map in ONE launch — what the demo does with cv2.line over a numpy mask for
//                       every stroke ever drawn, followed by a host-to-device copy (qt_demo_seg2cat.py:432-433, 459-463);
//   p3d_label_features  the label map straight to the activations of the Encoder's first layer: for a one-hot image b{res}.fromrgb (1x1 convolution, bias,
//                       lrelu) is the table lookup y[:, pixel] = T[:, label(pixel)], so the one-hot tensor, its casts and the convolution never exist.
//
// Strokes.  A work-group owns a tile of 16 rows x 16 row groups; a thread owns up to four consecutive pixels of one row.  The groups of a row are laid out from the
// DESTINATION's alignment as in frame_ops.hip (group 0 is the head in front of the row's first 4-byte boundary), so every full group is stored as one dword.  The
// stroke table is walked in chunks of 256: one thread tests one stroke's bounding box (grown by ceil(t / 2)) against the tile, the survivors are compacted into
// LDS in table order (wave64 ballot + prefix) and every thread walks that list for its pixels; the last covering stroke wins, which is painting in table order.
// The next chunk's stroke is loaded before the walk; no load sits under a per-lane branch (out-of-range strokes and pixels re-read a valid neighbour).
// Coverage is the integer capsule rule of include/p3d_hip.h.  With pixels in [0, 4095] and endpoints in [-4096, 8191]: |p| <= 8191 and |d| <= 12287 per
// component, so s, L and the cross product stay below 2^29 (int32) and 4 cross^2, t^2 L below 2^60 (int64).
#include "p3d_common.h"

namespace {

using namespace p3d;

constexpr int kChunk = 256;                         // strokes per pass = threads per work-group
constexpr int kTileRows = 16, kTileGroups = 16;

struct PaintArgs {
    const uint8_t* base; int64_t base_pitch;
    uint8_t* dst; int64_t dst_pitch;
    const int* strokes;                             // [K][6] = x0, y0, x1, y1, thickness, label
    int K, H, W, groups;
};

struct Stroke { int ax, ay, dx, dy, L, t2, label, pad; };      // 32 bytes: two 16-byte LDS reads, every lane the same address (a broadcast)

__global__ void __launch_bounds__(256) paint_strokes_kernel(const PaintArgs a)
{
    __shared__ Stroke list[kChunk];
    __shared__ int wave_hits[kChunk / kWave];

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int g = blockIdx.x * kTileGroups + (tid % kTileGroups);
    const int y = blockIdx.y * kTileRows + tid / kTileGroups;
    const int yc = min(y, a.H - 1);                                 // rows past the mask re-read the last row and store nothing
    uint8_t* const drow = a.dst + (int64_t)yc * a.dst_pitch;
    const int head = (int)((4 - (((uintptr_t)drow) & 3u)) & 3u);    // pixels in front of the row's first 4-byte boundary
    const int x0 = g == 0 ? 0 : head + 4 * (g - 1);
    const int x1 = g == 0 ? min(head, a.W) : min(a.W, x0 + 4);
    const int cnt = (y < a.H && g < a.groups) ? max(x1 - x0, 0) : 0;
    const int xb = min(x0, a.W - 1);

    unsigned lab[4];
    const uint8_t* const brow = a.base + (int64_t)yc * a.base_pitch;
#pragma unroll
    for (int i = 0; i < 4; ++i) lab[i] = brow[min(xb + i, a.W - 1)];

    // the tile's pixel rectangle, conservative in x (a row's head is at most three pixels)
    const int tx0 = max(0, 4 * ((int)blockIdx.x * kTileGroups - 1)), tx1 = min(a.W - 1, 4 * ((int)blockIdx.x * kTileGroups + kTileGroups) + 2);
    const int ty0 = blockIdx.y * kTileRows, ty1 = min(a.H - 1, ty0 + kTileRows - 1);

    int cur[6] = {};
    if (a.K > 0) {
        const int* p = a.strokes + (int64_t)min(tid, a.K - 1) * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) cur[k] = p[k];
    }
    for (int c0 = 0; c0 < a.K; c0 += kChunk) {
        const int r = (cur[4] + 1) >> 1;
        const bool hit = c0 + tid < a.K
                      && min(cur[0], cur[2]) - r <= tx1 && max(cur[0], cur[2]) + r >= tx0
                      && min(cur[1], cur[3]) - r <= ty1 && max(cur[1], cur[3]) + r >= ty0;
        Stroke s;
        s.ax = cur[0]; s.ay = cur[1]; s.dx = cur[2] - cur[0]; s.dy = cur[3] - cur[1];
        s.L = s.dx * s.dx + s.dy * s.dy; s.t2 = cur[4] * cur[4]; s.label = cur[5] & 255; s.pad = 0;
        {                                                           // the next chunk's stroke travels under this chunk's walk
            const int* p = a.strokes + (int64_t)min(c0 + kChunk + tid, a.K - 1) * 6;
#pragma unroll
            for (int k = 0; k < 6; ++k) cur[k] = p[k];
        }
        const unsigned long long ballot = __ballot(hit);
        if (lane == 0) wave_hits[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kChunk / kWave; ++w) {
            const int h = wave_hits[w];
            before += w < wave ? h : 0;
            total += h;
        }
        if (hit) list[before + __popcll(ballot & ((1ull << lane) - 1ull))] = s;
        __syncthreads();
        for (int j = 0; j < total; ++j) {
            const Stroke q = list[j];
            const int px = xb - q.ax, py = yc - q.ay;
            const int s0 = px * q.dx + py * q.dy;                   // p . d of the first pixel; the next ones add dx
            const int cr0 = px * q.dy - py * q.dx;                  // p x d; the next ones add dy
            const int64_t t2 = q.t2, t2L = t2 * (int64_t)q.L;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int si = s0 + i * q.dx, cri = cr0 + i * q.dy;
                const int64_t pxi = px + i, ex = pxi - q.dx, ey = py - q.dy;
                const int64_t d_a = 4 * (pxi * pxi + (int64_t)py * py);
                const int64_t d_b = 4 * (ex * ex + ey * ey);
                const int64_t d_l = 4 * ((int64_t)cri * cri);
                const bool cov = si <= 0 ? d_a <= t2 : (si >= q.L ? d_b <= t2 : d_l <= t2L);
                lab[i] = cov ? (unsigned)q.label : lab[i];
            }
        }
        __syncthreads();                                            // the list and the counts are rewritten by the next chunk
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

// ---- label map -> first-layer activations ----------------------------------------------------------------------------------------------
struct FeatArgs {
    const uint8_t* mask; int64_t mask_n, mask_row;
    const float* table;                              // [L + 1][C]; row L serves every byte >= L
    void* out; int64_t sn, sc, sy, sx;
    int N, H, W, L, C, cchunk;
};

template <class T> __device__ __forceinline__ void pack_store(T* p, const float (&v)[4]);
template <> __device__ __forceinline__ void pack_store<float>(float* p, const float (&v)[4]) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
template <> __device__ __forceinline__ void pack_store<__half>(__half* p, const float (&v)[4])
{
    const __half2 a = __floats2half2_rn(v[0], v[1]), b = __floats2half2_rn(v[2], v[3]);
    uint2 u; u.x = *(const unsigned*)&a; u.y = *(const unsigned*)&b;
    *(uint2*)p = u;
}
__device__ __forceinline__ void pack_store8(__half* p, const float (&v)[8])
{
    const __half2 a = __floats2half2_rn(v[0], v[1]), b = __floats2half2_rn(v[2], v[3]), c = __floats2half2_rn(v[4], v[5]), d = __floats2half2_rn(v[6], v[7]);
    uint4 u; u.x = *(const unsigned*)&a; u.y = *(const unsigned*)&b; u.z = *(const unsigned*)&c; u.w = *(const unsigned*)&d;
    *(uint4*)p = u;
}
template <class T, int V> __device__ __forceinline__ void store_vec(T* p, const float (&v)[V])
{
    if constexpr (V == 8) pack_store8(p, v);
    else pack_store<T>(p, v);
}

// the table into LDS, rows `pitch` floats apart (transposed: [C][pitch >= L + 1]): NL 16-byte loads per thread, all issued before the first is used (reads past the
// table re-read its last pack and are dropped), so staging is one memory round trip.  C % 4 == 0 keeps a pack inside one row.
template <int NL>
__device__ __forceinline__ void stage_table(float* lds, const FeatArgs& a, int pitch, bool transposed)
{
    const int packs = (a.L + 1) * a.C / 4;
    float4 v[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) v[i] = ((const float4*)a.table)[min((int)threadIdx.x + 256 * i, packs - 1)];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const int e = ((int)threadIdx.x + 256 * i) * 4;
        if (e < packs * 4) {
            const int l = e / a.C, c = e - l * a.C;
            if (transposed) {
                lds[c * pitch + l] = v[i].x; lds[(c + 1) * pitch + l] = v[i].y; lds[(c + 2) * pitch + l] = v[i].z; lds[(c + 3) * pitch + l] = v[i].w;
            } else {
                *(float4*)(lds + l * pitch + c) = v[i];
            }
        }
    }
    __syncthreads();
}

// channels-last destination (c stride 1): a thread owns V consecutive channels of four pixels; consecutive lanes hold consecutive channel packs of one pixel, then the
// next pixel — a wave instruction stores 1 KB of consecutive bytes.  The four labels are loaded before the first use.
template <class T, int V, int NL>
__global__ void __launch_bounds__(256) label_features_cl_kernel(const FeatArgs a)
{
    extern __shared__ __align__(16) float lds[];
    const int pitch = a.C + 4;                                       // rows a 16-byte read apart in the banks
    stage_table<NL>(lds, a, pitch, false);
    const int packs = a.C / V;
    const int64_t total = (int64_t)a.N * a.H * a.W * packs;
    const int64_t first = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    int lab[4], cp[4];
    int64_t off[4];
    bool live[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t e = first + 256 * i;
        live[i] = e < total;
        const int64_t ec = live[i] ? e : total - 1;
        const int64_t pix = ec / packs;
        cp[i] = (int)(ec - pix * packs) * V;
        const int x = (int)(pix % a.W);
        const int64_t row = pix / a.W;
        const int yy = (int)(row % a.H), n = (int)(row / a.H);
        lab[i] = a.mask[(int64_t)n * a.mask_n + (int64_t)yy * a.mask_row + x];
        off[i] = (int64_t)n * a.sn + (int64_t)yy * a.sy + (int64_t)x * a.sx + cp[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float* t = lds + min(lab[i], a.L) * pitch + cp[i];
        float v[V];
#pragma unroll
        for (int k = 0; k < V; k += 4) {
            const float4 q = *(const float4*)(t + k);
            v[k] = q.x; v[k + 1] = q.y; v[k + 2] = q.z; v[k + 3] = q.w;
        }
        if (live[i]) store_vec<T, V>((T*)a.out + off[i], v);
    }
}

// planar destination (x stride 1): a thread owns V consecutive pixels of one row for the channels [blockIdx.y * cchunk, + cchunk); consecutive lanes hold consecutive
// pixel packs, so per channel a wave instruction stores 1 KB of consecutive bytes.  The table is held transposed: lanes that differ in the label differ in the bank.
template <class T, int V, int NL>
__global__ void __launch_bounds__(256) label_features_planar_kernel(const FeatArgs a)
{
    extern __shared__ __align__(16) float lds[];
    const int pitch = a.L + 2;
    stage_table<NL>(lds, a, pitch, true);
    const int packs = (a.W + V - 1) / V;
    const int64_t total = (int64_t)a.N * a.H * packs;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = e < total;
    const int64_t ec = live ? e : total - 1;
    const int x0 = (int)(ec % packs) * V;
    const int64_t row = ec / packs;
    const int yy = (int)(row % a.H), n = (int)(row / a.H);
    const int cnt = min(V, a.W - x0);
    const uint8_t* m = a.mask + (int64_t)n * a.mask_n + (int64_t)yy * a.mask_row + x0;
    int lab[V];
#pragma unroll
    for (int i = 0; i < V; ++i) lab[i] = min((int)m[min(i, cnt - 1)], a.L);
    if (!live) return;
    T* const o = (T*)a.out + (int64_t)n * a.sn + (int64_t)yy * a.sy + x0;
    const int c0 = blockIdx.y * a.cchunk;
    for (int c = c0; c < c0 + a.cchunk; ++c) {
        float v[V];
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = lds[c * pitch + lab[i]];
        T* const p = o + (int64_t)c * a.sc;
        if (cnt == V) {
            store_vec<T, V>(p, v);
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (i < cnt) st<T>(p + i, v[i]);
        }
    }
}

// any other strides, or a destination the packs do not align in: one element per thread
template <class T, int NL>
__global__ void __launch_bounds__(256) label_features_strided_kernel(const FeatArgs a)
{
    extern __shared__ __align__(16) float lds[];
    const int pitch = a.C + 4;
    stage_table<NL>(lds, a, pitch, false);
    const int64_t total = (int64_t)a.N * a.H * a.W * a.C;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = e < total;
    const int64_t ec = live ? e : total - 1;
    const int x = (int)(ec % a.W);
    int64_t r = ec / a.W;
    const int yy = (int)(r % a.H); r /= a.H;
    const int c = (int)(r % a.C), n = (int)(r / a.C);
    const int lab = min((int)a.mask[(int64_t)n * a.mask_n + (int64_t)yy * a.mask_row + x], a.L);
    if (live) st<T>((T*)a.out + (int64_t)n * a.sn + (int64_t)c * a.sc + (int64_t)yy * a.sy + (int64_t)x * a.sx, lds[lab * pitch + c]);
}

} // namespace

extern "C" int p3d_paint_strokes(const uint8_t* base, int64_t base_row_pitch, uint8_t* dst, int64_t dst_row_pitch, int32_t h, int32_t w,
                                 const int32_t* strokes, int32_t n_strokes, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(base && dst, "paint_strokes: base and dst must be non-null");
    P3D_REQUIRE(h >= 1 && w >= 1 && h <= P3D_PAINT_MAX_SIZE && w <= P3D_PAINT_MAX_SIZE, "paint_strokes: the mask is 1 .. %d pixels a side (got %d x %d)", P3D_PAINT_MAX_SIZE, h, w);
    P3D_REQUIRE(n_strokes >= 0 && n_strokes <= P3D_PAINT_MAX_STROKES, "paint_strokes: 0 .. %d strokes (got %d)", P3D_PAINT_MAX_STROKES, n_strokes);
    P3D_REQUIRE(strokes || n_strokes == 0, "paint_strokes: %d strokes but no table", n_strokes);
    P3D_REQUIRE(base_row_pitch >= w && dst_row_pitch >= w, "paint_strokes: a row pitch is shorter than the row");
    P3D_REQUIRE(base != dst, "paint_strokes: the mask is written out of place");
    PaintArgs a;
    a.base = base; a.base_pitch = base_row_pitch; a.dst = dst; a.dst_pitch = dst_row_pitch; a.strokes = strokes;
    a.K = n_strokes; a.H = h; a.W = w; a.groups = (w + 3) / 4 + 1;
    const dim3 grid((unsigned)ceil_div(a.groups, kTileGroups), (unsigned)ceil_div(h, kTileRows));
    hipLaunchKernelGGL(paint_strokes_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    count_launch(FAM_AUX);
    return check_launch("paint_strokes");
}

extern "C" int p3d_label_features(const uint8_t* mask, int64_t mask_frame_pitch, int64_t mask_row_pitch, const float* table, int32_t n_labels,
                                  void* out, int32_t dtype, const int64_t* out_stride, int32_t n, int32_t c, int32_t h, int32_t w, p3d_stream_t stream)
{
    using namespace p3d;
    P3D_REQUIRE(mask && table && out && out_stride, "label_features: mask, table, out and out_stride must be non-null");
    P3D_REQUIRE(((uintptr_t)table & 15u) == 0, "label_features: the table must be 16-byte aligned");
    P3D_REQUIRE(dtype == P3D_F32 || dtype == P3D_F16, "label_features: out is fp32 or fp16");
    P3D_REQUIRE(n >= 1 && h >= 1 && w >= 1 && c >= 4 && c % 4 == 0, "label_features: sizes must be positive and C a multiple of 4 (C = %d)", c);
    P3D_REQUIRE(n_labels >= 1 && n_labels <= 255, "label_features: 1 .. 255 labels (got %d)", n_labels);
    P3D_REQUIRE(mask_row_pitch >= w && (n == 1 || mask_frame_pitch >= (int64_t)h * mask_row_pitch), "label_features: the mask leaves its pitches");
    for (int t = 0; t < 4; ++t) P3D_REQUIRE(out_stride[t] >= 0, "label_features: negative output stride");
    const int64_t lds_floats = (int64_t)(n_labels + 1) * (c + 4) + 4 * (int64_t)c;       // covers both layouts: [L + 1][C + 4] and [C][L + 2]
    P3D_REQUIRE(lds_floats * 4 <= 64 * 1024, "label_features: the table ((%d + 1) x %d) does not fit 64 KB of LDS", n_labels, c);
    FeatArgs a;
    a.mask = mask; a.mask_n = mask_frame_pitch; a.mask_row = mask_row_pitch; a.table = table; a.out = out;
    a.sn = out_stride[0]; a.sc = out_stride[1]; a.sy = out_stride[2]; a.sx = out_stride[3];
    a.N = n; a.H = h; a.W = w; a.L = n_labels; a.C = c; a.cchunk = c % 16 == 0 ? 16 : 4;
    const size_t lds = (size_t)lds_floats * 4;
    const bool small_table = (n_labels + 1) * c <= 2 * 256 * 4;                           // table packs per thread: 2 (the shipped label sets at C = 64) or 16 (the 64 KB bound)
#define P3D_LAUNCH_NL(kernel, grid, ...) do { if (small_table) hipLaunchKernelGGL((kernel<__VA_ARGS__, 2>), grid, dim3(256), lds, s, a); \
                                              else hipLaunchKernelGGL((kernel<__VA_ARGS__, 16>), grid, dim3(256), lds, s, a); } while (0)
    const hipStream_t s = (hipStream_t)stream;
    const int esize = dtype == P3D_F32 ? 4 : 2;
    const uintptr_t op = (uintptr_t)out;
    const int64_t elements = (int64_t)n * c * h * w;
    auto aligned = [&](int v, int64_t s0, int64_t s1, int64_t s2) { return op % 16 == 0 && s0 % v == 0 && s1 % v == 0 && s2 % v == 0; };
    if (a.sc == 1) {
        const int v = (dtype == P3D_F16 && c % 8 == 0) ? 8 : 4;
        if (aligned(16 / esize, a.sn, a.sy, a.sx)) {
            const int64_t blocks = (elements / v + 1023) / 1024;
            P3D_REQUIRE(blocks < (1ll << 31), "label_features: too many elements");
            if (dtype == P3D_F32) P3D_LAUNCH_NL(label_features_cl_kernel, dim3((unsigned)blocks), float, 4);
            else if (v == 8)      P3D_LAUNCH_NL(label_features_cl_kernel, dim3((unsigned)blocks), __half, 8);
            else                  P3D_LAUNCH_NL(label_features_cl_kernel, dim3((unsigned)blocks), __half, 4);
            count_launch(FAM_AUX);
            return check_launch("label_features");
        }
    } else if (a.sx == 1) {
        const int v = 16 / esize;
        if (aligned(v, a.sn, a.sc, a.sy)) {
            const int64_t blocks = ((int64_t)n * h * ((w + v - 1) / v) + 255) / 256;
            P3D_REQUIRE(blocks < (1ll << 31), "label_features: too many elements");
            const dim3 grid((unsigned)blocks, (unsigned)(c / a.cchunk));
            if (dtype == P3D_F32) P3D_LAUNCH_NL(label_features_planar_kernel, grid, float, 4);
            else                  P3D_LAUNCH_NL(label_features_planar_kernel, grid, __half, 8);
            count_launch(FAM_AUX);
            return check_launch("label_features");
        }
    }
    const int64_t blocks = (elements + 255) / 256;
    P3D_REQUIRE(blocks < (1ll << 31), "label_features: too many elements");
    if (dtype == P3D_F32) P3D_LAUNCH_NL(label_features_strided_kernel, dim3((unsigned)blocks), float);
    else                  P3D_LAUNCH_NL(label_features_strided_kernel, dim3((unsigned)blocks), __half);
    count_launch(FAM_AUX);
    return check_launch("label_features");
}
#undef P3D_LAUNCH_NL
