// Shared host/device helpers for libp3d_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <atomic>
#include "../../include/p3d_hip.h"

namespace p3d {

constexpr int kWave = 64;                       // gfx950 wavefront
constexpr int kNumCU = 256;                     // MI355X
enum Family { FAM_BIAS_ACT = 0, FAM_UPFIRDN = 1, FAM_FLRELU = 2, FAM_RENDER = 3, FAM_CONV = 4, FAM_AUX = 5, FAM_COUNT = 6 };

void  set_error(const char* fmt, ...);
int   fail(int code, const char* fmt, ...);
void  count_launch(int family);
int   check_launch(const char* what);         // hipGetLastError -> status

template <class T> struct Acc            { typedef float  type; };
template <>        struct Acc<double>    { typedef double type; };

template <class T> __device__ __forceinline__ typename Acc<T>::type ld(const T* p)            { return (typename Acc<T>::type)(*p); }
template <>        __device__ __forceinline__ float ld<__half>(const __half* p)                 { return __half2float(*p); }
template <class T> __device__ __forceinline__ void st(T* p, typename Acc<T>::type v)          { *p = (T)v; }
template <>        __device__ __forceinline__ void st<__half>(__half* p, float v)               { *p = __float2half(v); }

// One-time opt-in to more than 64 KB of dynamic LDS for kernel `fn`, once PER DEVICE (the attribute belongs to the device's
// code object: a process that drives several GPUs must set it on each); `done` holds one bit per device ordinal.
inline hipError_t reserve_lds_once(const void* fn, int bytes, std::atomic<uint64_t>& done)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
    return e;
}

// ---- forward convolution host path (csrc/conv2d.hip; DESIGN.md "Conv forward host path") ------------------------------------------------
// One call of the p3d_conv2d_nhwc* family (and of p3d_conv2d_forward / _bwd_data once their weights are laid out), filled by name.
struct ConvRequest {
    // the convolution: all plan_conv reads besides the facts below
    int dtype = P3D_F32;
    int32_t n_img = 0, h = 0, wdt = 0, ci = 0, co = 0;
    int64_t w_img_stride = 0;
    int32_t kernel_size = 3, resample = 0;     // 0: "same"; 1: transposed, stride 2; 2: valid, stride 2
    int32_t act = 0;
    float gain = 1.f, clamp = -1.f;
    int32_t out_h = 0, out_w = 0;              // transposed form only, 0 = 2h+1 / 2w+1: the output size conv_transpose2d's output_padding asks for (2h+1 or 2h+2); the extra
                                               // row / column only sees taps that fall outside the input, i.e. comes out as zeros, as in the reference's op
    int32_t x_split = 0, y_split = 0;          // P3D_F32_BF16X3 only: the activations are / the result is to be in the bf16x3 K-row layout — per pixel and 32 channels
                                               // [32 x bf16 hi | 32 x bf16 lo] in the 128 bytes of 32 floats.  Every route takes x_split; y_split needs a 3x3 halo kernel
    // the operands: read by launch_conv_plan only
    const void* x = nullptr; const void* w = nullptr; void* y = nullptr;
    const float* bias = nullptr; const float* noise = nullptr; const float* noise_strength = nullptr;
    const void* zeros128 = nullptr;
    const float* in_scale = nullptr; const float* out_scale = nullptr;        // ConvArgs::iscale / oscale
    void* workspace = nullptr; int64_t workspace_bytes = 0;                   // split-K scratch, or null
    p3d_stream_t stream = nullptr;
    // what the plan may know about the operands
    bool has_in_scale = false, has_out_scale = false;
    bool y_aligned = true;                     // y on a 16-byte boundary: gates the h2 routes
    bool have_ws = false;                      // a workspace came with the call: a short 3x3 grid may prefer the generic kernel and its split K
    int64_t ws_usable_bytes = 0;               // ... and this much of it is usable (0 when it is misaligned): split K is granted when its scratch fits

    void note_operands()                       // the facts of a real call
    {
        has_in_scale = in_scale != nullptr; has_out_scale = out_scale != nullptr; y_aligned = (((uintptr_t)y) & 15u) == 0;
        have_ws = workspace != nullptr && workspace_bytes > 0;
        ws_usable_bytes = (workspace != nullptr && (((uintptr_t)workspace) & 15u) == 0) ? workspace_bytes : 0;
    }
    void assume_plain_operands()               // the facts the sizing entry points assume: aligned pointers, all the workspace the plan wants, no scales
    {
        has_in_scale = has_out_scale = false; y_aligned = have_ws = true; ws_usable_bytes = INT64_MAX;
    }
};

// What a request runs: plan_conv decides, launch_conv_plan only obeys.
struct ConvPlan {
    int route = 0;                             // enum p3d_conv_route
    int variant = 0;                           // template instantiation within the route's kernel family (ConvVariant, conv2d.hip)
    int grid[3] = {0, 0, 0};                   // (generic: z = images x classes x ksplit)
    int fold = 0, cls_major = 0, co64 = 0, ksplit = 1, y_split = 0;          // as stored into ConvArgs
    int64_t scratch_bytes = 0;                 // split-K scratch the route would like, granted or not (0: none)
};

int plan_conv(const ConvRequest& r, ConvPlan* plan);                         // pure host: geometry checks + the route decision; no launch, no device API
int launch_conv_plan(const ConvRequest& r, const ConvPlan& plan);            // operand checks, ConvArgs, the launches
inline int run_conv(ConvRequest& r)
{
    r.note_operands();
    ConvPlan plan;
    const int rc = plan_conv(r, &plan);
    return rc != P3D_OK ? rc : launch_conv_plan(r, plan);
}

// 4 x 4 transpose of one dword per (lane of a quad, register): on return register c of quad lane t holds what register t of quad lane c held.  Two DPP stages:
// lane ^ 1 inside the register pairs (0, 1), (2, 3), then lane ^ 2 inside (0, 2), (1, 3).  What turns the MFMA accumulator layout (a lane = ONE output channel,
// four consecutive GEMM rows in registers 4 q .. 4 q + 3) into "a lane = four consecutive channels of one row": 16-byte stores instead of four 4-byte (or 2-byte) ones.
__device__ __forceinline__ void quad_transpose4(unsigned (&w)[4], const bool odd1, const bool odd2)
{
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
        const unsigned send = odd1 ? w[2 * pr] : w[2 * pr + 1];
        const unsigned recv = (unsigned)__builtin_amdgcn_mov_dpp((int)send, 0xB1, 0xF, 0xF, true);      // quad_perm [1, 0, 3, 2]
        w[2 * pr]     = odd1 ? recv : w[2 * pr];
        w[2 * pr + 1] = odd1 ? w[2 * pr + 1] : recv;
    }
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
        const unsigned send = odd2 ? w[pr] : w[pr + 2];
        const unsigned recv = (unsigned)__builtin_amdgcn_mov_dpp((int)send, 0x4E, 0xF, 0xF, true);      // quad_perm [2, 3, 0, 1]
        w[pr]     = odd2 ? recv : w[pr];
        w[pr + 2] = odd2 ? w[pr + 2] : recv;
    }
}

static inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

} // namespace p3d

#define P3D_REQUIRE(cond, ...) do { if (!(cond)) return p3d::fail(P3D_ERR_ARGUMENT, __VA_ARGS__); } while (0)
