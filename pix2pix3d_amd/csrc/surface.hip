// Surface casting for gfx950: geometry frames straight from the density field, beside the lattice + marching cubes + rasterizer
// pipeline (applications/extract_mesh.py:60-99; shape.hip, mesh_raster.hip) and without its R^3 evaluations.
//
// p3d_surface_cast: per ray the first sample t_i = near + i dt whose density exceeds the threshold, B bisection steps between it and
// the sample before, and the central density differences at the point found (include/p3d_hip.h has the contract, operation by
// operation).  The lattice kernel (shape.hip, lattice_sigma_kernel) with rays for a driver: the gather and the density net are
// render_device.h's, fed `coord_scale * p` exactly as there, so every density equals p3d_sample_points' sigma at the same point bit
// for bit and the whole cast equals the same procedure composed over the point kernel.
//
// Mapping: a wave owns 32 rays — lane (j, h) = (lane & 31, lane >> 5) holds ray j of the tile, the two halves gather channels
// [16 h, 16 h + 16) and keep IDENTICAL ray state (mlp_sigma's cross-half sum is commutative, both halves see the same density).  The
// march, the bisection and the six gradient evaluations are wave-uniform loops: mlp_layer1's MFMAs and mlp_sigma's cross-half
// reduction need the full EXEC mask, so no lane branches round an evaluation — a ray that has finished, or a lane past the end of the
// rays, evaluates the box centre (always a valid gather, and lines every such lane shares) and ignores the result.  The march ends
// when a ballot shows no ray of the wave still searching, the later phases are skipped by a wave without a hit.  With raster_width a
// tile is an 8 x 4 pixel block (8 rows, 4 columns), so the rays of a wave end together and their taps share lines; outputs are
// indexed by ray either way.  Persistent grid: one grid row per ray set, about two blocks per CU over the launch, as the lattice.
//
// p3d_surface_shade: one thread per pixel, fp64, mesh_tri.h's headlight rule with the density gradient for a normal.
//
// p3d_surface_occlusion: the second ray stage — from every hit point short rays into the hemisphere the surface faces (ambient occlusion) or
// towards a light (shadows); per point the number of directions it uses and the number of those that reach the end unblocked.  Same tile
// mapping, same densities.  Each lane keeps a PRIVATE cursor (direction k, step j): every wave-uniform iteration evaluates each lane's own
// current sample, and a lane whose ray is decided moves to its next used direction in a loop that holds no evaluation (so it may diverge).
// No lane sits through a direction it does not use, neighbours whose hemispheres differ do not stall each other; the wave runs for as
// long as its busiest lane.  The set's direction table sits in LDS behind the decoder copy.
// p3d_surface_shade_lit: the shade with a directional light, an ambient-occlusion pair and a shadow pair, each optional.
#include "density_device.h"
#include "render_host.h"

namespace p3d {

struct CastArgs {
    float near, dt, threshold, eps, half_box;
    int steps, refine, raster;                       // raster: R when the M rays of a set are an R x R image (R % 8 == 0), else 0
    unsigned rays_per_set;
    uint8_t* hit; float* depth; float* position; float* grad;
};

// One individually rounded fp32 operation each.  Plain operators under contract(off), NOT __fmul_rn / __fadd_rn / __fsub_rn: in this
// toolchain those are header functions whose bodies (x * y, x + y) are compiled contractable, and once inlined hipcc fuses them into
// v_fma_f32 whatever the caller's pragma says (seen in this kernel's ISA); an operator written under the pragma carries no contract flag.
__device__ __forceinline__ float mul_rn(float a, float b)
{
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b)
{
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b)
{
#pragma clang fp contract(off)
    return a - b;
}
// o + t d, per component: one rounded product, one rounded sum (never an fma)
__device__ __forceinline__ float ray_at(float o, float t, float d) { return add_rn(o, mul_rn(t, d)); }
__device__ __forceinline__ float sample_t(float near, int i, float dt) { return add_rn(near, mul_rn((float)i, dt)); }
__device__ __forceinline__ float midpoint(float lo, float hi) { return mul_rn(0.5f, add_rn(lo, hi)); }
// (a NaN component is not outside: the comparison is false)
__device__ __forceinline__ bool outside_box(float half_box, float x, float y, float z)
{
    return half_box > 0.f && (fabsf(x) > half_box || fabsf(y) > half_box || fabsf(z) > half_box);
}

template <int NNETS>
__global__ void __launch_bounds__(kWavesPerBlock * 64, 2)
surface_cast_kernel(RenderArgs a, CastArgs c)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    stage_decoder(lds, a.decoder);
    __syncthreads();
    constexpr int SN = NNETS - 1;
    const rsrc_t rsrc = plane_rsrc(a);
    const unsigned set = blockIdx.y;                                 // one ray set per grid row
    const unsigned img_off = set * a.img_bytes;                      // (0 for every set when the planes are shared)
    const unsigned M = c.rays_per_set, tiles = (M + 31) / 32;
    const size_t base = (size_t)set * M;
    const unsigned tiles_x = c.raster > 0 ? (unsigned)c.raster / 4u : 1u;
    for (unsigned t = blockIdx.x * kWavesPerBlock + wave; t < tiles; t += gridDim.x * kWavesPerBlock) {
        const unsigned q = tile_point(t, j, c.raster, tiles_x);
        const bool live = q < M;
        const size_t g = base + (live ? q : M - 1);
        const float ox = a.ray_o[g * 3], oy = a.ray_o[g * 3 + 1], oz = a.ray_o[g * 3 + 2];
        const float dx = a.ray_d[g * 3], dy = a.ray_d[g * 3 + 1], dz = a.ray_d[g * 3 + 2];

        // ---- march: the first sample above the threshold ----
        bool searching = live, found = false, bisect = false;
        float lo = c.near, hi = c.near;
#pragma unroll 1
        for (int i = 0; i < c.steps; ++i) {
            if (__ballot(searching) == 0ull) break;
            const float ti = sample_t(c.near, i, c.dt);
            const float px = ray_at(ox, ti, dx), py = ray_at(oy, ti, dy), pz = ray_at(oz, ti, dz);
            const bool use = searching && !outside_box(c.half_box, px, py, pz);
            const float s = sigma_at<SN>(a, rsrc, img_off, lds, lane, h, use ? px : 0.f, use ? py : 0.f, use ? pz : 0.f);
            if (use && s > c.threshold) { found = true; searching = false; bisect = i > 0; hi = ti; }
            else if (searching) lo = ti;
        }
        // ---- bisection between the last sample below and the first above ----
        if (__ballot(bisect) != 0ull) {
#pragma unroll 1
            for (int b = 0; b < c.refine; ++b) {
                const float tm = midpoint(lo, hi);
                const float px = ray_at(ox, tm, dx), py = ray_at(oy, tm, dy), pz = ray_at(oz, tm, dz);
                const bool use = bisect && !outside_box(c.half_box, px, py, pz);
                const float s = sigma_at<SN>(a, rsrc, img_off, lds, lane, h, use ? px : 0.f, use ? py : 0.f, use ? pz : 0.f);
                if (bisect) { if (use && s > c.threshold) hi = tm; else lo = tm; }
            }
        }
        const float depth = found ? hi : INFINITY;
        const float wx = found ? ray_at(ox, hi, dx) : 0.f, wy = found ? ray_at(oy, hi, dy) : 0.f, wz = found ? ray_at(oz, hi, dz) : 0.f;
        const bool store = live && h == 0;
        if (store) {
            c.hit[g] = found ? 1 : 0;
            c.depth[g] = depth;
            if (c.position) { c.position[g * 3] = wx; c.position[g * 3 + 1] = wy; c.position[g * 3 + 2] = wz; }
        }
        // ---- gradient: central differences of the density at the point found (no box clip) ----
        if (c.grad) {
            if (__ballot(found) != 0ull) {
                float sp = 0.f;
#pragma unroll 1
                for (int k = 0; k < 6; ++k) {                        // (+x, -x, +y, -y, +z, -z): only component k >> 1 moves, x - eps as x + (-eps)
                    const int ax = k >> 1;
                    const float e = (k & 1) ? -c.eps : c.eps;
                    const float s = sigma_at<SN>(a, rsrc, img_off, lds, lane, h, ax == 0 ? add_rn(wx, e) : wx, ax == 1 ? add_rn(wy, e) : wy,
                                                 ax == 2 ? add_rn(wz, e) : wz);
                    if (!(k & 1)) sp = s;
                    else if (store) c.grad[g * 3 + ax] = found ? sub_rn(sp, s) : 0.f;
                }
            } else if (store) {
                c.grad[g * 3] = 0.f; c.grad[g * 3 + 1] = 0.f; c.grad[g * 3 + 2] = 0.f;
            }
        }
    }
}

struct OcclusionArgs {
    float ds, threshold, half_box;
    int n_dirs, steps, raster;
    unsigned points_per_set;
    const uint8_t* active; const float* directions;  // [N*M], [N][K][3]; origins and facings travel as RenderArgs' ray_o, ray_d
    uint8_t* open; uint8_t* total;
};

constexpr int kMaxDirections = 255;                  // the counts are bytes; 255 * 3 floats of LDS behind the decoder copy

// facing . d > 0: three rounded products, two rounded sums, left to right (a NaN compares false)
__device__ __forceinline__ bool faces(float fx, float fy, float fz, const float* d)
{
    return add_rn(add_rn(mul_rn(fx, d[0]), mul_rn(fy, d[1])), mul_rn(fz, d[2])) > 0.f;
}

template <int NNETS>
__global__ void __launch_bounds__(kWavesPerBlock * 64, 2)
surface_occlusion_kernel(RenderArgs a, OcclusionArgs c)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const unsigned set = blockIdx.y;                                 // one point set, and its direction table, per grid row
    float* dirs = lds + kDecoderFloats;
    stage_decoder(lds, a.decoder);
    for (int i = threadIdx.x; i < c.n_dirs * 3; i += blockDim.x) dirs[i] = c.directions[(size_t)set * c.n_dirs * 3 + i];
    __syncthreads();
    constexpr int SN = NNETS - 1;
    const rsrc_t rsrc = plane_rsrc(a);
    const unsigned img_off = set * a.img_bytes;                      // (0 for every set when the planes are shared)
    const unsigned M = c.points_per_set, tiles = (M + 31) / 32;
    const size_t base = (size_t)set * M;
    const unsigned tiles_x = c.raster > 0 ? (unsigned)c.raster / 4u : 1u;
    const int K = c.n_dirs, last = c.steps - 1;
    for (unsigned t = blockIdx.x * kWavesPerBlock + wave; t < tiles; t += gridDim.x * kWavesPerBlock) {
        const unsigned q = tile_point(t, j, c.raster, tiles_x);
        const bool live = q < M;
        const size_t g = base + (live ? q : M - 1);
        const float ox = a.ray_o[g * 3], oy = a.ray_o[g * 3 + 1], oz = a.ray_o[g * 3 + 2];
        const float fx = a.ray_d[g * 3], fy = a.ray_d[g * 3 + 1], fz = a.ray_d[g * 3 + 2];
        const bool on = live && c.active[g] != 0;

        // ---- the directions this point uses; the cursor starts at the first of them (K: none, or none left) ----
        int total = 0, k = K;
        if (on)
            for (int i = K - 1; i >= 0; --i)
                if (faces(fx, fy, fz, dirs + i * 3)) { ++total; k = i; }
        int open = 0, step = 0;
        bool entered = false;                                        // the current ray has had a sample inside the box
        const int bound = K * c.steps;                               // (<= 255 * 4096) no lane has more samples than this
#pragma unroll 1
        for (int it = 0; it < bound; ++it) {
            const bool work = k < K;
            if (__ballot(work) == 0ull) break;
            const float* d = dirs + (work ? k : 0) * 3;
            const float s = mul_rn((float)(step + 1), c.ds);
            const float px = ray_at(ox, s, d[0]), py = ray_at(oy, s, d[1]), pz = ray_at(oz, s, d[2]);
            const bool out = outside_box(c.half_box, px, py, pz);
            const bool use = work && !out;
            const float sg = sigma_at<SN>(a, rsrc, img_off, lds, lane, h, use ? px : 0.f, use ? py : 0.f, use ? pz : 0.f);
            if (work) {
                const bool blocked = use && sg > c.threshold;        // (a NaN density never blocks)
                // every component of the point is monotone in the step: a ray that was inside the box and has left it stays outside
                const bool left = out && entered;
                if (blocked || left || step == last) {
                    if (!blocked) ++open;
                    do ++k; while (k < K && !faces(fx, fy, fz, dirs + k * 3));      // no evaluation in here: free to diverge
                    step = 0; entered = false;
                } else {
                    ++step; entered = entered || !out;
                }
            }
        }
        if (live && h == 0) { c.open[g] = (uint8_t)open; c.total[g] = (uint8_t)total; }
    }
}

// ---- what the two ray stages' entry points share ---------------------------------------------------------------------------------
// The descriptor of a ray (or point) stage: one set of rays_per_img per grid row, shared planes honoured.
static int stage_check_desc(const p3d_render_desc* d, const char* who)
{
    const int rc = check_plane_desc(d, who, true, true);
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(d->rays_per_img >= 1, "%s: rays_per_img must be >= 1 (got %d)", who, d->rays_per_img);
    return P3D_OK;
}

// The tile mapping's limits (`what` a set holds: rays, points).
static int stage_check_tiles(const p3d_render_desc* d, int32_t raster_width, const char* who, const char* what)
{
    const int64_t M = d->rays_per_img;
    P3D_REQUIRE(raster_width >= 0 && (raster_width == 0 || (raster_width % 8 == 0 && (int64_t)raster_width * raster_width == M)),
                "%s: raster_width %d must be 0, or a multiple of 8 whose square is rays_per_img (%d)", who, raster_width, d->rays_per_img);
    if (M > (int64_t)INT32_MAX - 31)
        return fail(P3D_ERR_UNSUPPORTED, "%s: %lld %s per set do not fit the kernel's 32-bit in-set index", who, (long long)M, what);
    return P3D_OK;
}

// One launch over all sets of a checked descriptor (n_img >= 1); origins and directions (or facings) travel as RenderArgs' ray_o, ray_d.
template <class StageArgs>
static int stage_launch(void (*one_net)(RenderArgs, StageArgs), void (*two_nets)(RenderArgs, StageArgs), const p3d_render_desc* d, const float* planes_cl,
                        const float* decoder, const float* ray_o, const float* ray_d, const StageArgs& c, size_t lds_floats, p3d_stream_t stream,
                        const char* who)
{
    RenderArgs a{};
    fill_plane_args(a, d, true);
    a.planes = planes_cl; a.decoder = decoder; a.ray_o = ray_o; a.ray_d = ray_d;
    hipLaunchKernelGGL(d->n_nets == 1 ? one_net : two_nets, set_row_grid(d->rays_per_img, d->n_img), dim3(kWavesPerBlock * 64), lds_floats * sizeof(float),
                       (hipStream_t)stream, a, c);
    count_launch(FAM_RENDER);
    return check_launch(who);
}

// ---- shading ----------------------------------------------------------------------------------------------------------------
constexpr double kSurfaceGrey = 200.0;               // P3D_MESH_GREY

__device__ __forceinline__ uint8_t byte_of(double v)
{
    return (uint8_t)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));
}

// One thread per pixel.  mode 1: the normal map.  mode 0: light [F][3] (null: the headlight), ao_* and sh_* [F*H*W] counts (null pairs: 1);
// with all three null this is the plain lambert shade: amb * 1.0 and b * 1.0 are exact.
__global__ void __launch_bounds__(256) surface_shade_kernel(const uint8_t* __restrict__ hit, const float* __restrict__ grad, const uint8_t* __restrict__ albedo,
                                                            const float* __restrict__ cam2world, const float* __restrict__ light,
                                                            const uint8_t* __restrict__ ao_open, const uint8_t* __restrict__ ao_total,
                                                            const uint8_t* __restrict__ sh_open, const uint8_t* __restrict__ sh_total, int64_t total,
                                                            int64_t per_frame, float ambient, int mode, int bg_r, int bg_g, int bg_b, uint8_t* __restrict__ rgb)
{
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    uint8_t* dst = rgb + p * 3;
    if (!hit[p]) { dst[0] = (uint8_t)bg_r; dst[1] = (uint8_t)bg_g; dst[2] = (uint8_t)bg_b; return; }
    const float g32[3] = {grad[p * 3], grad[p * 3 + 1], grad[p * 3 + 2]};
    const bool finite = isfinite(g32[0]) && isfinite(g32[1]) && isfinite(g32[2]);
    const double g0 = finite ? (double)g32[0] : 0.0, g1 = finite ? (double)g32[1] : 0.0, g2 = finite ? (double)g32[2] : 0.0;
    double nn = g0 * g0; nn = nn + g1 * g1; nn = nn + g2 * g2;
    if (mode == 1) {                                                 // normal map: -g / |g| in [0, 255]; no direction -> 128
        const double n = sqrt(nn);
        const double gs[3] = {g0, g1, g2};
        for (int k = 0; k < 3; ++k) {
            const double u = n > 0.0 ? -gs[k] / n : 0.0;
            dst[k] = byte_of(floor((u * 0.5 + 0.5) * 255.0 + 0.5));
        }
        return;
    }
    const int64_t frame = p / per_frame;
    const float* v = light ? light + frame * 3 : nullptr;            // the light, or the camera's forward axis
    const float* cam = cam2world + frame * 16;
    const double l0 = (double)(v ? v[0] : cam[2]), l1 = (double)(v ? v[1] : cam[6]), l2 = (double)(v ? v[2] : cam[10]);
    double ll = l0 * l0; ll = ll + l1 * l1; ll = ll + l2 * l2;
    double dot = g0 * l0; dot = dot + g1 * l1; dot = dot + g2 * l2;
    const double den = sqrt(nn) * sqrt(ll);
    double cosv = 0.0;
    if (den > 0.0) {
        if (light) { const double c = -dot / den; cosv = c > 0.0 ? c : 0.0; }       // n = -g / |g|: the side that faces the light (NaN: 0)
        else cosv = fabs(dot) / den;
    }
    const double ao = ao_total && ao_total[p] > 0 ? (double)ao_open[p] / (double)ao_total[p] : 1.0;
    const double sh = sh_total && sh_total[p] > 0 ? (double)sh_open[p] / (double)sh_total[p] : 1.0;
    const double amb = (double)ambient;
    const double lit_ambient = amb * ao;
    double lit_direct = (1.0 - amb) * cosv;
    lit_direct = lit_direct * sh;
    const double shade = lit_ambient + lit_direct;
    for (int k = 0; k < 3; ++k) {
        const double alb = albedo ? (double)albedo[p * 3 + k] : kSurfaceGrey;
        dst[k] = byte_of(floor(alb * shade + 0.5));
    }
}

// The launch behind p3d_surface_shade and p3d_surface_shade_lit, whose frame sizes and required pointers are checked the same way.
static int shade_launch(const char* who, const uint8_t* hit, const float* grad, const uint8_t* albedo, const float* cam2world, const float* light,
                        const uint8_t* ao_open, const uint8_t* ao_total, const uint8_t* sh_open, const uint8_t* sh_total, int32_t n_frames, int32_t height,
                        int32_t width, float ambient, int32_t mode, int32_t bg_r, int32_t bg_g, int32_t bg_b, uint8_t* rgb, p3d_stream_t stream)
{
    if (n_frames == 0) return P3D_OK;
    P3D_REQUIRE(hit && grad && cam2world && rgb, "%s: null pointer", who);
    const int64_t per_frame = (int64_t)height * width, total = per_frame * n_frames;
    const int64_t blocks = (total + 255) / 256;
    if (blocks > INT32_MAX)
        return fail(P3D_ERR_UNSUPPORTED, "%s: %lld pixels are more than one launch takes", who, (long long)total);
    hipLaunchKernelGGL(surface_shade_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, hit, grad, albedo, cam2world, light, ao_open,
                       ao_total, sh_open, sh_total, total, per_frame, ambient, mode, bg_r & 255, bg_g & 255, bg_b & 255, rgb);
    count_launch(FAM_AUX);
    return check_launch(who);
}

} // namespace p3d

using namespace p3d;

extern "C" int p3d_surface_cast(const float* planes_cl, const float* decoder, const p3d_render_desc* d, const float* ray_o, const float* ray_d,
                                float near, float dt, int32_t steps, int32_t refine, float threshold, float eps, float half_box, int32_t raster_width,
                                uint8_t* hit, float* depth, float* position, float* grad, p3d_stream_t stream)
{
    int rc = stage_check_desc(d, "surface_cast");
    if (rc != P3D_OK) return rc;
    P3D_REQUIRE(planes_cl && decoder && ray_o && ray_d && hit && depth, "surface_cast: null pointer");
    if (steps < 2 || steps > 4096 || refine < 0 || refine > 24)
        return fail(P3D_ERR_UNSUPPORTED, "surface_cast: needs 2 <= steps <= 4096 and 0 <= refine <= 24 (got %d, %d)", steps, refine);
    rc = stage_check_tiles(d, raster_width, "surface_cast", "rays");
    if (rc != P3D_OK || d->n_img == 0) return rc;
    CastArgs c{};
    c.near = near; c.dt = dt; c.threshold = threshold; c.eps = eps; c.half_box = half_box;
    c.steps = steps; c.refine = refine; c.raster = raster_width; c.rays_per_set = (unsigned)d->rays_per_img;
    c.hit = hit; c.depth = depth; c.position = position; c.grad = grad;
    return stage_launch(surface_cast_kernel<1>, surface_cast_kernel<2>, d, planes_cl, decoder, ray_o, ray_d, c, kDecoderFloats, stream, "surface_cast");
}

extern "C" int p3d_surface_shade(const uint8_t* hit, const float* grad, const uint8_t* albedo, const float* cam2world, int32_t n_frames, int32_t height,
                                 int32_t width, float ambient, int32_t mode, int32_t bg_r, int32_t bg_g, int32_t bg_b, uint8_t* rgb, p3d_stream_t stream)
{
    P3D_REQUIRE(n_frames >= 0 && height >= 1 && width >= 1, "surface_shade: bad frame size %d x %d x %d", n_frames, height, width);
    P3D_REQUIRE(mode == 0 || mode == 1, "surface_shade: mode must be 0 (lambert) or 1 (normal), got %d", mode);
    return shade_launch("surface_shade", hit, grad, albedo, cam2world, nullptr, nullptr, nullptr, nullptr, nullptr, n_frames, height, width, ambient, mode,
                        bg_r, bg_g, bg_b, rgb, stream);
}

extern "C" int p3d_surface_occlusion(const float* planes_cl, const float* decoder, const p3d_render_desc* d, const float* origin, const float* facing,
                                     const uint8_t* active, const float* directions, int32_t n_directions, float ds, int32_t steps, float threshold,
                                     float half_box, int32_t raster_width, uint8_t* open, uint8_t* total, p3d_stream_t stream)
{
    int rc = stage_check_desc(d, "surface_occlusion");
    if (rc != P3D_OK) return rc;
    if (n_directions < 1 || n_directions > kMaxDirections || steps < 1 || steps > 4096)
        return fail(P3D_ERR_UNSUPPORTED, "surface_occlusion: needs 1 <= directions <= %d and 1 <= steps <= 4096 (got %d, %d)", kMaxDirections, n_directions,
                    steps);
    P3D_REQUIRE(planes_cl && decoder && origin && facing && active && directions && open && total, "surface_occlusion: null pointer");
    rc = stage_check_tiles(d, raster_width, "surface_occlusion", "points");
    if (rc != P3D_OK || d->n_img == 0) return rc;
    OcclusionArgs c{};
    c.ds = ds; c.threshold = threshold; c.half_box = half_box;
    c.n_dirs = n_directions; c.steps = steps; c.raster = raster_width; c.points_per_set = (unsigned)d->rays_per_img;
    c.active = active; c.directions = directions; c.open = open; c.total = total;
    return stage_launch(surface_occlusion_kernel<1>, surface_occlusion_kernel<2>, d, planes_cl, decoder, origin, facing, c, kDecoderFloats + kMaxDirections * 3,
                        stream, "surface_occlusion");
}

extern "C" int p3d_surface_shade_lit(const uint8_t* hit, const float* grad, const uint8_t* albedo, const float* cam2world, const float* light,
                                     const uint8_t* ao_open, const uint8_t* ao_total, const uint8_t* sh_open, const uint8_t* sh_total, int32_t n_frames,
                                     int32_t height, int32_t width, float ambient, int32_t bg_r, int32_t bg_g, int32_t bg_b, uint8_t* rgb,
                                     p3d_stream_t stream)
{
    P3D_REQUIRE(n_frames >= 0 && height >= 1 && width >= 1, "surface_shade_lit: bad frame size %d x %d x %d", n_frames, height, width);
    P3D_REQUIRE(!ao_open == !ao_total && !sh_open == !sh_total, "surface_shade_lit: an open count and its total come as a pair");
    return shade_launch("surface_shade_lit", hit, grad, albedo, cam2world, light, ao_open, ao_total, sh_open, sh_total, n_frames, height, width, ambient, 0,
                        bg_r, bg_g, bg_b, rgb, stream);
}
