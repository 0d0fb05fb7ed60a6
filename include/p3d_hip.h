/*
 * p3d_hip.h — C ABI of libp3d_hip.so, the MI355X (gfx950) kernel library behind the
 * pix2pix3D generator/renderer hot path.
 *
 * Plain C: raw device pointers, explicit sizes/strides, an explicit hipStream_t (passed as
 * void*), no torch types.  Every entry point
 *   - borrows its inputs, writes into caller-allocated outputs (the caller keeps ownership,
 *     normally torch's caching allocator),
 *   - enqueues on the given stream and returns without host synchronisation,
 *   - returns P3D_OK (0) or a negative error code; never throws across the boundary;
 *     p3d_last_error() gives the message for the calling thread,
 *   - keeps no mutable global device state (filters / MLP weights are kernel arguments or LDS
 *     copies, never device globals), so concurrent streams are safe.
 *
 * Each declaration cites the reference interface it stands in for (paths relative to the
 * reference checkout).  INTEGRATION.md shows the ctypes binding used on the Python side.
 */
#ifndef P3D_HIP_H
#define P3D_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* p3d_stream_t;              /* hipStream_t */

enum p3d_status {
    P3D_OK              =  0,
    P3D_ERR_UNSUPPORTED = -1,            /* "no specialised kernel": same meaning as return_code -1 of
                                            filtered_lrelu_plugin (filtered_lrelu.cpp:56-60) */
    P3D_ERR_ARGUMENT    = -2,
    P3D_ERR_LAUNCH      = -3
};

enum p3d_dtype { P3D_F32 = 0, P3D_F16 = 1, P3D_F64 = 2,
                 P3D_F32_BF16X3 = 3     /* conv entry points only: fp32 tensors, fp32 accumulation, every product formed as three bf16
                                           products of (hi, lo) splits — ~2^-16 relative per product at up to 5x the fp32 matrix rate;
                                           weights come from p3d_modulate_weights with the same code ([32 x hi | 32 x lo] K rows)      */,
                 P3D_F32_BF16X6 = 4     /* conv entry points only (p3d_conv2d_nhwc*, p3d_conv2d_forward / _bwd_data / _bwd_weight*): fp32 tensors AND fp32 weights in the
                                           P3D_F32 layouts, fp32 accumulation; every operand is split IN REGISTERS into three bf16 pieces (hi + mid + lo = the
                                           fp32 value exactly: 3 x 8 significand bits) and every product formed as the six bf16 products of magnitude
                                           >= 2^-16 (hh, hm, mh, hl, lh, mm; the three dropped ones are <= 2^-23 relative together: the size of one fp32
                                           rounding) — fp32-accurate products at 6/16 of the f32-input MFMA's time, on the pipe that overlaps vector work */ };

/* ---- library services ------------------------------------------------------------------- */
const char* p3d_last_error(void);        /* message of the last failure on this host thread      */
int         p3d_abi_version(void);       /* bumped whenever a signature below changes            */
uint64_t    p3d_launch_count(void);      /* kernels enqueued by this library since load (tests use
                                            it to prove the HIP path ran, not a fallback)        */
/* per-kernel-family counters: which = 0 bias_act, 1 upfirdn2d, 2 filtered_lrelu, 3 render,
 * 4 conv/modconv, 5 layout/aux */
uint64_t    p3d_launch_count_of(int which);

/* ---- bias_act ---------------------------------------------------------------------------
 * Replaces bias_act_plugin.bias_act (torch_utils/ops/bias_act.cpp:36-94, kernel bias_act.cu:27-151).
 *   grad = 0: y = clamp(act(x + b[(i / step_b) % size_b]) * gain)
 *   grad = 1: x carries dy; xref/yref are the saved forward input/output; y = d/dx
 *   grad = 2: second-order term; dy carries the first-order upstream gradient
 * act: 1 linear, 2 relu, 3 lrelu, 4 tanh, 5 sigmoid, 6 elu, 7 selu, 8 softplus, 9 swish
 * (bias_act.py:23-33).  clamp < 0 disables clamping.  Null b/xref/yref/dy mean "absent"
 * (the plugin's empty tensor).  All tensors share x's dense layout; size_x <= INT32_MAX.   */
int p3d_bias_act(const void* x, const void* b, const void* xref, const void* yref, const void* dy,
                 void* y, int dtype, int grad, int act, float alpha, float gain, float clamp,
                 int64_t size_x, int32_t size_b, int64_t step_b, p3d_stream_t stream);

/* ---- upfirdn2d --------------------------------------------------------------------------
 * Replaces upfirdn2d_plugin.upfirdn2d (torch_utils/ops/upfirdn2d.cpp:20-102, kernels
 * upfirdn2d.cu:33-204): zero-insert upsample, pad/crop, 2-D FIR, decimate, per (n, c) image.
 * Sizes are {W, H, C, N}; strides (in elements) use the same order so NCHW and channels_last
 * both work.  f is fp32 [fh, fw] with element strides f_stride = {x, y}.  The caller computes
 * out size = (in*up + pad0 + pad1 - f + down) / down (upfirdn2d.cpp:39-40); only pad0 is needed
 * here.  flip = 0 convolves (filter mirrored), flip = 1 correlates.                          */
int p3d_upfirdn2d(const void* x, const float* f, void* y, int dtype,
                  const int32_t in_size[4], const int64_t in_stride[4],
                  const int32_t f_size[2], const int64_t f_stride[2],
                  const int32_t out_size[4], const int64_t out_stride[4],
                  int32_t up_x, int32_t up_y, int32_t down_x, int32_t down_y,
                  int32_t pad_x0, int32_t pad_y0, int32_t flip, float gain, p3d_stream_t stream);
/* p3d_upfirdn2d that ADDS its result into y (y += upfirdn2d(x)): the skip-image sum of SynthesisBlock (training/networks_stylegan2.py:453-459:
 * img = upsample2d(img) + torgb) from the upsampling launch.  Channels-last tensors, 4-tap filters, C a multiple of 16 bytes; anything else
 * P3D_ERR_UNSUPPORTED.                                                                                                          */
int p3d_upfirdn2d_acc(const void* x, const float* f, void* y, int dtype,
                  const int32_t in_size[4], const int64_t in_stride[4],
                  const int32_t f_size[2], const int64_t f_stride[2],
                  const int32_t out_size[4], const int64_t out_stride[4],
                  int32_t up_x, int32_t up_y, int32_t down_x, int32_t down_y,
                  int32_t pad_x0, int32_t pad_y0, int32_t flip, float gain, p3d_stream_t stream);

/* ---- filtered_lrelu ----------------------------------------------------------------------------
 * Replaces filtered_lrelu_plugin.filtered_lrelu (torch_utils/ops/filtered_lrelu.cpp:20-213; kernel parameters filtered_lrelu.h:18-72,
 * kernels filtered_lrelu.cu:143-1103):  y = fir_down( clamp( lrelu( fir_up(x + b) * up^2 * gain ) ) )  per (n, c) plane, in one pass.
 * Sizes are {W, H, C, N} and strides (in elements) use the same order.  fu / fd: dense fp32 tables [f_h][f_w] (a separable filter is
 * passed as its outer product, an absent one as the 1x1 table {1}).  The caller computes the sizes exactly as the plugin does
 * (filtered_lrelu.cpp:73-97): up-sampled extent c = x*up + pad0 + pad1 - (fu-1), y = (c - (fd-1) + down-1) / down, and for the sign
 * tensor s_h = y_h*down - (down-1) + (fd_h-1), active width likewise, rounded up to 16 elements, 4 elements per byte.
 * sign_mode 0: none.  1: WRITE the sign tensor s (uint8 [N][C][s_height][s_width_bytes], contiguous): element (x, y) of the up-sampled
 *   grid -> byte ((x + s_ofs_x) >> 2) of row (y + s_ofs_y), bits ((x + s_ofs_x) & 3) * 2: 0 passed, 1 negative (IEEE sign bit, as
 *   filtered_lrelu.cu:497-500), 2 clamped.  2: READ it instead of comparing (the backward configuration, filtered_lrelu.py:240-270):
 *   code & 1 -> times slope, code & 2 -> 0, elements outside the tensor pass unchanged; clamp is not applied.
 * sw_limit: valid bytes per sign row ((active width + 3) >> 2).  clamp = +inf disables clamping.
 * Returns P3D_ERR_UNSUPPORTED (-1, the plugin's "no specialised kernel" code, filtered_lrelu.cpp:56-60) when the tiles of this geometry
 * do not fit gfx950's 160 KB of LDS or s_ofs_x is not a multiple of 4 in write mode: the caller then takes the generic route
 * (upfirdn2d -> p3d_filtered_lrelu_act -> upfirdn2d), as the reference does.                                                        */
int p3d_filtered_lrelu(const void* x, const float* fu, const float* fd, const void* b, uint8_t* s, void* y, int dtype,
                       const int32_t x_size[4], const int64_t x_stride[4], const int32_t y_size[4], const int64_t y_stride[4], int64_t b_stride,
                       int32_t fu_w, int32_t fu_h, int32_t fd_w, int32_t fd_h, int32_t up, int32_t down, int32_t pad_x0, int32_t pad_y0,
                       int32_t s_width_bytes, int32_t s_height, int32_t s_ofs_x, int32_t s_ofs_y, int32_t sw_limit,
                       float gain, float slope, float clamp, int32_t flip_filters, int32_t sign_mode, p3d_stream_t stream);
/* filtered_lrelu_plugin.filtered_lrelu_act_ (filtered_lrelu.cpp:217-296, kernel filtered_lrelu.cu:1109-1213): in place on x (fp16, fp32
 * or fp64):  x = clamp(lrelu(x * gain)).  sign_mode 1 writes s [N][C][H][s_width/4] with s_width = W rounded up to 16 ELEMENTS (code 1
 * when the scaled value is < 0 — not the sign bit: the two kernels differ on -0.0, filtered_lrelu.cu:1140-1149); sign_mode 2 reads s
 * [N][C][s_height][s_width/4] at (x + s_ofs_x, y + s_ofs_y), elements outside pass with the gain only.                              */
int p3d_filtered_lrelu_act(void* x, uint8_t* s, int dtype, const int32_t x_size[4], const int64_t x_stride[4],
                           int32_t s_width, int32_t s_height, int32_t s_ofs_x, int32_t s_ofs_y, float gain, float slope, float clamp,
                           int32_t sign_mode, p3d_stream_t stream);

/* ---- fused tri-plane ray-marcher -----------------------------------------------------------
 * Stands in for the tensor-op pipeline of training/volumetric_rendering:
 *   ImportanceRenderer.forward   renderer.py:88-140   (p3d_render_forward)
 *   ImportanceRenderer.run_model renderer.py:142-148  (p3d_sample_points)
 *   sample_importance/sample_pdf renderer.py:194-253  (p3d_importance_sample, also fused above)
 *   MipRayMarcher2.run_forward   ray_marcher.py:25-57 (fused)
 * with the OSG decoders (training/triplane.py:112-135 one net; training/triplane_cond.py:926-970
 * two nets, density from the second) evaluated on the f32 MFMA path.  Random numbers are inputs
 * (the host draws them exactly where the reference would: renderer.py:190, :237).            */
#define P3D_RENDER_SHARED_PLANES 2
typedef struct p3d_render_desc {
    int32_t n_img;                        /* N                                                  */
    int32_t rays_per_img;                 /* M (ignored by p3d_sample_points)                   */
    int32_t plane_h, plane_w;             /* tri-plane resolution; 32 channels per plane        */
    int32_t n_nets;                       /* 1: OSGDecoder, 2: OSGDecoder_semantic_lateSeparate */
    int32_t semantic_sigmoid;             /* 2-net decoder: squash the label channels too       */
    int32_t depth_resolution;             /* S_c  rendering_options['depth_resolution']         */
    int32_t depth_resolution_importance;  /* S_f                                                */
    int32_t disparity_space_sampling;
    int32_t white_back;
    float   ray_start, ray_end;           /* used when t_start/t_end are null                   */
    float   box_warp;
    /* plane memory layout, in floats; all 0 = the default [N][3][H][W][32].  Texel (n, p, y, x) starts at
     * n*image_stride + p*plane_stride + (y*W + x)*pixel_stride and holds 32 contiguous channels; e.g. a
     * channels-last backbone output [N][H][W][96] is (image H*W*96, plane 32, pixel 96).                 */
    int64_t image_stride, plane_stride, pixel_stride;
    int32_t raster_order;                 /* != 0: ray m of an image is pixel (m / R, m % R) of an R x R raster (R*R = rays_per_img):
                                             lets the kernel assign 16 x 16 pixel blocks to workgroups for L2 locality.
                                             Bit 1 (P3D_RENDER_SHARED_PLANES; p3d_render_forward / _dual / _debug, p3d_surface_cast and p3d_surface_occlusion;
                                             every other entry point ignores it): the plane tensor holds ONE
                                             image that all n_img ray sets read (many cameras of one latent) — the strides describe that one image  */
    int32_t mlp_bf16x3;                   /* p3d_render_forward only, != 0: the decoder stream comes from p3d_pack_decoder_bf16x3 and the MLPs run
                                             as three bf16 MFMAs per fp32 product (hi/lo splits, fp32 accumulation: ~5e-6 of the hidden range per
                                             layer) instead of f32-input MFMAs at 1/16 of that rate.  0 = exact fp32 (p3d_pack_decoder).
                                             2: the stream comes from p3d_pack_decoder_l1x6 and LAYER 1 of every net runs as six bf16 MFMAs
                                             per product of three-piece splits (fp32-accurate, csrc/bf16_split.h); layer 2 stays on the
                                             f32-input MFMA (its third weight image does not fit the LDS).                                   */
} p3d_render_desc;

int p3d_render_decoder_floats(void);     /* size of the packed decoder stream, in floats        */

/* planes [N][96][H][W] (backbone output, NCHW) -> [N][3][H][W][32]: one 128-byte line per texel */
int p3d_planes_to_channels_last(const float* planes_nchw, float* planes_cl, int32_t n_img, int32_t h, int32_t w,
                                p3d_stream_t stream);

/* FullyConnectedLayer weights (networks_stylegan2.py:96-130; w1 [64,32], b1 [64], w2 [33,64],
 * b2 [33], raw parameters: the lr_mul / sqrt(fan_in) gains are applied here) -> MFMA operand
 * stream.  Net a = colour net, net b = label+density net (null for the single-net decoder).   */
int p3d_pack_decoder(const float* w1_a, const float* b1_a, const float* w2_a, const float* b2_a,
                     const float* w1_b, const float* b1_b, const float* w2_b, const float* b2_b,
                     int32_t n_nets, float lr_mul, float* packed, p3d_stream_t stream);
/* the same parameters in the operand order of the bf16x3 decoder (p3d_render_desc.mlp_bf16x3); same size, fp32 values */
int p3d_pack_decoder_bf16x3(const float* w1_a, const float* b1_a, const float* w2_a, const float* b2_a,
                            const float* w1_b, const float* b1_b, const float* w2_b, const float* b2_b,
                            int32_t n_nets, float lr_mul, float* packed, p3d_stream_t stream);

/* the same parameters with layer 1 in the bf16 operand order and layer 2 in the f32-MFMA order (p3d_render_desc.mlp_bf16x3 == 2); same size, fp32 values */
int p3d_pack_decoder_l1x6(const float* w1_a, const float* b1_a, const float* w2_a, const float* b2_a,
                          const float* w1_b, const float* b1_b, const float* w2_b, const float* b2_b,
                          int32_t n_nets, float lr_mul, float* packed, p3d_stream_t stream);

/* ray_o, ray_d [N*M][3]; u_coarse [N*M][S_c] and u_fine [N*M][S_f] uniforms in [0,1);
 * t_start/t_end optional per-ray limits [N*M] ('auto' ray range), null otherwise.
 * Outputs: feat [N*M][32*n_nets] (already *2-1), depth [N*M] (clamped to the global sample-depth
 * range, ray_marcher.py:49-50), wsum [N*M].  minmax_ws: 2 x uint32 device scratch.
 * dbg_fine [N*M][S_f] (sorted importance depths) and dbg_wcoarse [N*M][S_c-1] are optional.
 * Returns P3D_ERR_UNSUPPORTED when S_c or S_f exceed 64 (or S_f == 0).
 * Envelope: at most 64 coarse and 1..64 fine samples per ray; clamp_mode 'softplus' (the only mode ray_marcher.py:35 accepts); no
 * density_noise term (renderer.py:116-117: training-time regulariser, 0 in every shipped configuration); the OSG 32-64-33 decoders.
 * Outside it the Python mirror takes the tensor-op formulation and says so with a RuntimeWarning (or raises under fused_policy 'require'). */
int p3d_render_forward(const float* planes_cl, const float* decoder, const float* ray_o, const float* ray_d,
                       const float* u_coarse, const float* u_fine, const float* t_start, const float* t_end,
                       const p3d_render_desc* desc, float* feat, float* depth, float* wsum, uint32_t* minmax_ws,
                       float* dbg_fine, float* dbg_wcoarse, p3d_stream_t stream);
/* The same launch (same kernel instantiation) with one more optional record: dbg_bins [N*M][S_f] <- for every importance draw, in draw order,
 * the index torch.searchsorted(cdf, u, right=True) returns in sample_pdf (renderer.py:221-253) — the integers behind dbg_fine, so that the index
 * work of the FUSED launch can be compared exactly (tests/test_render_gpu.py), not only that of the stand-alone p3d_importance_sample_index. */
int p3d_render_forward_debug(const float* planes_cl, const float* decoder, const float* ray_o, const float* ray_d,
                             const float* u_coarse, const float* u_fine, const float* t_start, const float* t_end,
                             const p3d_render_desc* desc, float* feat, float* depth, float* wsum, uint32_t* minmax_ws,
                             float* dbg_fine, float* dbg_wcoarse, int32_t* dbg_bins, p3d_stream_t stream);

/* ---- two plane sets: ImportanceSemanticRenderer (training/volumetric_rendering/renderer.py:256-438) --------------------------------
 * The renderer of TriPlaneSemanticGenerator (training/triplane_cond.py:746-758): a texture and a semantic tri-plane set of the same
 * size and layout.  The label decoder (OSGDecoder_semantic, FC 32-64-33) reads the semantic planes' features and gives density +
 * 32 label channels; the colour decoder (OSGDecoder over 64 inputs, FC 64-64-33, density row unused) reads cat(texture, semantic)
 * features (renderer.py:324-333).  Sampling, merging and compositing are ImportanceRenderer's over cat(colour, label): outputs as
 * p3d_render_forward with n_nets = 2 (feat [N*M][64]; desc->semantic_sigmoid squashes the labels too).  Inference only.
 * p3d_pack_decoder_dual: raw FullyConnectedLayer parameters (w1_tex [64][64], b1_tex [64], w2_tex [33][64], b2_tex [33]; w1_sem [64][32],
 * ...) -> p3d_render_decoder_floats_dual() floats.  p3d_sample_points_dual = run_model: rgb [N*P][64] = cat(colour, label), sigma [N*P]. */
int p3d_render_decoder_floats_dual(void);
int p3d_pack_decoder_dual(const float* w1_tex, const float* b1_tex, const float* w2_tex, const float* b2_tex,
                          const float* w1_sem, const float* b1_sem, const float* w2_sem, const float* b2_sem,
                          float lr_mul, float* packed, p3d_stream_t stream);
int p3d_render_forward_dual(const float* planes_tex_cl, const float* planes_sem_cl, const float* decoder_dual, const float* ray_o, const float* ray_d,
                            const float* u_coarse, const float* u_fine, const float* t_start, const float* t_end,
                            const p3d_render_desc* desc, float* feat, float* depth, float* wsum, uint32_t* minmax_ws, p3d_stream_t stream);
int p3d_sample_points_dual(const float* planes_tex_cl, const float* planes_sem_cl, const float* decoder_dual, const float* coords,
                           const p3d_render_desc* desc, int32_t pts_per_img, float* rgb, float* sigma, p3d_stream_t stream);

/* ---- backward of p3d_render_forward (training configs) ------------------------------------------
 * What autograd derives for ImportanceRenderer.forward (renderer.py:88-140) in the reference, as two recomputing launches
 * (csrc/render_bwd.hip): the forward sweep again, driven by g_feat, hands every sample its compositing scalars on a tape; a
 * point-wise pass re-evaluates gather + MLPs per sample and back-propagates on the matrix cores.  Importance depths are constants
 * (renderer.py:198, 211).  Gradients w.r.t. the rays and w.r.t. the depth output are not produced (the training losses use
 * neither; the host falls back to the tensor-op formulation if asked for them).
 *   decoder_bwd : p3d_render_bwd_decoder_floats() floats from p3d_pack_decoder_bwd (same raw parameters as p3d_pack_decoder)
 *   g_feat [N*M][32*n_nets] = dL/dfeat, g_wsum [N*M] = dL/dwsum or null; rays / uniforms / limits exactly as in the forward call
 *   tape_intervals [N*M][S-1][4], tape_samples [N*M][S][4] fp32 scratch (S = S_c + S_f), 16-byte aligned
 *   d_planes_cl [N][3][H][W][32] <- dL/dplanes (channels-last, zeroed here, accumulated with atomics)
 *   d_decoder [p3d_render_grad_decoder_floats()] <- per net (stride 4260 floats): dW1 [64][32] @0, db1 [64] @2048, dW2 [33][64]
 *   @2112, db2 [33] @4224, gradients of the EFFECTIVE weights w * lr_mul / sqrt(fan_in), b * lr_mul (multiply by the same gains
 *   for the raw parameters).                                                                                              */
int p3d_render_bwd_decoder_floats(void);
int p3d_render_grad_decoder_floats(void);
int p3d_pack_decoder_bwd(const float* w1_a, const float* w2_a, const float* w1_b, const float* w2_b, int32_t n_nets, float lr_mul,
                         float* packed_bwd, p3d_stream_t stream);
int p3d_render_backward(const float* planes_cl, const float* decoder, const float* decoder_bwd, const float* ray_o, const float* ray_d,
                        const float* u_coarse, const float* u_fine, const float* t_start, const float* t_end,
                        const p3d_render_desc* desc, const float* g_feat, const float* g_wsum, float* tape_intervals, float* tape_samples,
                        float* d_planes_cl, float* d_decoder, p3d_stream_t stream);

/* coords [N*P][3] -> rgb [N*P][32*n_nets], sigma [N*P]  (G.sample / G.sample_mixed, extract_mesh) */
int p3d_sample_points(const float* planes_cl, const float* decoder, const float* coords, const p3d_render_desc* desc,
                      int32_t pts_per_img, float* rgb, float* sigma, p3d_stream_t stream);
/* Backward of p3d_sample_points: what autograd derives for ImportanceRenderer.run_model (renderer.py:142-148: grid_sample + decoder)
 * when G.sample_mixed is differentiated — the density regularisation of training/loss.py:681-706 ('Greg' phase).  One launch: per
 * point gather + MLPs again, MLP backward on the matrix cores, plane gradient by whole-texel atomics (the point-wise half of
 * p3d_render_backward, no tape).  g_rgb [N*P][32*n_nets] = dL/drgb (post-activation outputs), g_sigma [N*P] = dL/dsigma; either may
 * be null (= zero).  d_planes_cl / d_decoder / decoder_bwd exactly as in p3d_render_backward.  Coordinates receive no gradient.        */
int p3d_sample_points_backward(const float* planes_cl, const float* decoder, const float* decoder_bwd, const float* coords,
                               const p3d_render_desc* desc, int32_t pts_per_img, const float* g_rgb, const float* g_sigma,
                               float* d_planes_cl, float* d_decoder, p3d_stream_t stream);

/* ---- shape extraction (applications/extract_mesh.py:60-99, csrc/shape.hip) ---------------------------
 * p3d_sample_lattice: get_sigma_field_np (extract_mesh.py:60-81) in one launch.  sigma [N][nx][ny][nz] <- the density at the point
 * (xs[i], ys[j], zs[k]) of image n, for N = desc->n_img <= 65535 and nx*ny*nz <= 2^32 - 32; xs / ys / zs are device tables of nx / ny / nz
 * floats.  Planes, decoder (p3d_pack_decoder, exact fp32) and desc as for p3d_sample_points; only the density net runs (net 0 of
 * OSGDecoder, net 1 of OSGDecoder_semantic_lateSeparate), and the values equal p3d_sample_points' sigma at the same points.
 * P3D_ERR_UNSUPPORTED when the planes exceed the 32-bit byte offsets of the kernel's buffer descriptor.                        */
int p3d_sample_lattice(const float* planes_cl, const float* decoder, const p3d_render_desc* desc, const float* xs, const float* ys,
                       const float* zs, int32_t nx, int32_t ny, int32_t nz, float* sigma, p3d_stream_t stream);

/* Marching cubes (the role of mcubes.marching_cubes in extract_mesh.py:89) on a float32 field u [X][Y][Z] (contiguous, every
 * dimension >= 2).  A corner is inside when u > threshold.  Output contract:
 *   vertices float32 [V][3], in index space: one per lattice edge whose ends straddle the threshold, at the lower end (i, j, k) plus t
 *     along the edge's axis a, t = (threshold - u_lower) / (u_upper - u_lower); numbered by lower corner in row-major order, then by a;
 *   faces int64 [F][3]: by cube in row-major order, then in the order of the case table (csrc/mc_tables.h, generated by
 *     pix2pix3d_amd/mc_table.py; ambiguous faces separate their two inside corners, so this is not the original Lorensen table);
 *     (b - a) x (c - a) points from inside to outside.  No atomics: the output is a pure function of (u, threshold).
 * Three steps, on one stream:
 *   1. p3d_marching_cubes_classify: mask [X*Y*Z] uint8 (bit a: the edge along axis a is crossed), cases [X*Y*Z] uint8 (the case of
 *      the cube whose lower corner this is, 0 when there is none), block_counts int32 [2][B] (vertices, then triangles, of every
 *      block of 256 corners; B = p3d_marching_cubes_blocks(X, Y, Z));
 *   2. the caller's exclusive scans of the two rows -> block_voff, block_foff int64 [B], and the totals V and F ON THE HOST (a
 *      device-to-host copy: this sequence cannot be captured into a graph);
 *   3. p3d_marching_cubes_emit: vbase int32 [X*Y*Z] scratch, vertices, faces.  P3D_ERR_UNSUPPORTED when V > INT32_MAX (32-bit vertex ids). */
int64_t p3d_marching_cubes_blocks(int32_t X, int32_t Y, int32_t Z);
int p3d_marching_cubes_classify(const float* u, int32_t X, int32_t Y, int32_t Z, float threshold, uint8_t* mask, uint8_t* cases,
                                int32_t* block_counts, p3d_stream_t stream);
int p3d_marching_cubes_emit(const float* u, int32_t X, int32_t Y, int32_t Z, float threshold, const uint8_t* mask, const uint8_t* cases,
                            const int64_t* block_voff, const int64_t* block_foff, int64_t n_vertices, int64_t n_faces,
                            int32_t* vbase, float* vertices, int64_t* faces, p3d_stream_t stream);

/* ---- surface casting (csrc/surface.hip) -------------------------------------------------------------------------------------
 * A geometry view without a mesh.  Stands beside the pipeline of applications/extract_mesh.py:60-99 (density lattice, marching cubes,
 * then a rasterizer: R^3 decoder evaluations before the first pixel): the level set {sigma > threshold} is found along the camera's
 * rays only, up to its first crossing.
 * p3d_surface_cast: N = desc->n_img ray sets of M = desc->rays_per_img rays, one launch; ray_o, ray_d [N*M][3] as for
 *   p3d_render_forward; planes, decoder (p3d_pack_decoder, exact fp32) and desc as for p3d_sample_lattice, and bit 1 of
 *   desc->raster_order (P3D_RENDER_SHARED_PLANES) is honoured: one plane set serves the N ray sets.  Only the density net runs (net
 *   n_nets - 1: layer 1 and the sigma row); sigma(p) below is bit for bit what p3d_sample_points returns at p.
 *   The contract is fp32, every operation individually rounded (no fused multiply-add):
 *     samples   t_i = near + float(i) * dt, i = 0 .. steps - 1 (the caller computes dt = float32((far - near) / (steps - 1)) once);
 *               p(t) = o + t * d per component;
 *     box clip  half_box > 0: a point with any |component| > half_box is OUTSIDE — it is not above the threshold and no decoder
 *               result is used for it (march and bisection alike); half_box <= 0: no clip;
 *     hit       the first i with sigma(p(t_i)) > threshold.  i = 0: depth = t_0.  Else lo = t_{i-1}, hi = t_i and `refine` times
 *               tm = 0.5 * (lo + hi); sigma(p(tm)) > threshold ? hi = tm : lo = tm; then depth = hi;
 *     gradient  position = o + depth * d; grad[a] = sigma(position + eps e_a) - sigma(position - eps e_a): one subtraction per axis,
 *               unnormalised, only component a of the point moves, no box clip.  grad is NOT finite at every hit: a decoder may
 *               return non-finite densities, and a position can overflow fp32;
 *     miss      hit = 0, depth = +inf, position = grad = 0.  A NaN density is never above the threshold.
 *   Outputs: hit uint8 [N*M], depth float [N*M], position and grad float [N*M][3] (either may be null).
 *   raster_width = R > 0 (R * R = M, R % 8 == 0): a wave takes an 8 x 4 pixel block instead of 32 consecutive rays — scheduling only,
 *   the outputs are indexed by ray and have the same bytes.
 *   Limits: 2 <= steps <= 4096, 0 <= refine <= 24 (else P3D_ERR_UNSUPPORTED), n_nets 1 or 2, N <= 65535, and p3d_sample_lattice's
 *   32-bit plane addressing limits (P3D_ERR_UNSUPPORTED).  No GPU work on an error.
 * p3d_surface_shade: rgb uint8 [F][H][W][3] from hit [F*H*W], grad [F*H*W][3], albedo uint8 [F*H*W][3] (null: P3D_MESH_GREY) and
 *   cam2world float [F][16] (row-major 4x4; entries 2, 6, 10 are the camera's forward axis f).  fp64, products summed left to right,
 *   no contraction — p3d_mesh_shade's headlight rule with the density gradient g for a normal:
 *     mode 0 (lambert)  cos = |g.f| / (|g| |f|), 0 where the denominator is 0; shade = ambient + (1 - ambient) cos;
 *                       byte = floor(albedo * shade + 0.5) clamped to [0, 255];
 *     mode 1 (normal)   byte_k = floor((-g_k / |g| * 0.5 + 0.5) * 255 + 0.5); |g| = 0: 128 in every component.
 *   A gradient with a non-finite component counts as the zero gradient in both modes.  hit == 0: the background colour.
 * p3d_surface_occlusion: the second ray stage — what short rays from points ON the surface find.  N = desc->n_img point sets of
 *   M = desc->rays_per_img points, one launch: origin, facing float [N*M][3], active uint8 [N*M], directions float [N][K][3] (per set:
 *   a camera-attached light differs per view), K = n_directions.  planes, decoder, desc, P3D_RENDER_SHARED_PLANES, raster_width and
 *   sigma(p) exactly as for p3d_surface_cast.  The contract is fp32, every operation individually rounded (no fused multiply-add):
 *     samples   s_j = float(j + 1) * ds, j = 0 .. steps - 1 (the caller computes ds = float32(reach / steps) once);
 *               p = o + s_j * d per component: one rounded product, one rounded sum;
 *     used      direction k is USED by point p iff active[p] != 0 and ((f_x d_x) + (f_y d_y)) + (f_z d_z) > 0: three rounded products,
 *               two rounded sums in that order (a NaN makes the comparison false);
 *     blocked   a used direction is BLOCKED iff for some j the point is inside the box (p3d_surface_cast's clip: half_box > 0 and any
 *               |component| > half_box is outside; half_box <= 0 clips nothing) and sigma(point) > threshold.  A NaN density never
 *               blocks;
 *     outputs   total[p] = the number of used directions, open[p] = the number of used directions that are not blocked; uint8 [N*M],
 *               both 0 for an inactive point.
 *   No value depends on which points share a launch or a wave.  (Every component of p is monotone in j, so a ray that has been inside
 *   the box and has left it cannot be blocked any more; the kernel stops it there.)
 *   Limits: 1 <= n_directions <= 255, 1 <= steps <= 4096 (else P3D_ERR_UNSUPPORTED), and p3d_surface_cast's descriptor checks and
 *   raster_width rule.  No GPU work on an error.
 * p3d_surface_shade_lit: p3d_surface_shade's mode 0 with a light, an ambient-occlusion pair and a shadow pair, each optional (null).
 *   light float [F][3]: the world-space direction TOWARDS the light of every frame; ao_open / ao_total and sh_open / sh_total uint8
 *   [F*H*W]: p3d_surface_occlusion's counts (a pair is given whole or not at all).  fp64, products summed left to right, no contraction:
 *     v      = light of the frame, or without one the camera's forward axis f;
 *     nn     = g.g, ll = v.v, dot = g.v, den = sqrt(nn) * sqrt(ll)   (a gradient with a non-finite component counts as zero);
 *     cos    = 0 where den > 0 is false; with a light max(0, -dot / den) (the normal is n = -g / |g|: cos = n.l / |l|; NaN -> 0); without
 *              one |dot| / den (p3d_surface_shade's headlight);
 *     ao     = ao_total > 0 ? ao_open / ao_total : 1 (1 without the pair); sh likewise from the shadow pair;
 *     shade  = (ambient * ao) + (((1 - ambient) * cos) * sh);  byte = floor(albedo * shade + 0.5) clamped to [0, 255].
 *   hit == 0: the background colour.  With no light and no pair the bytes are p3d_surface_shade's (mode 0).                        */
int p3d_surface_cast(const float* planes_cl, const float* decoder, const p3d_render_desc* desc, const float* ray_o, const float* ray_d,
                     float near, float dt, int32_t steps, int32_t refine, float threshold, float eps, float half_box, int32_t raster_width,
                     uint8_t* hit, float* depth, float* position, float* grad, p3d_stream_t stream);
int p3d_surface_shade(const uint8_t* hit, const float* grad, const uint8_t* albedo, const float* cam2world, int32_t n_frames, int32_t height,
                      int32_t width, float ambient, int32_t mode, int32_t bg_r, int32_t bg_g, int32_t bg_b, uint8_t* rgb, p3d_stream_t stream);
int p3d_surface_occlusion(const float* planes_cl, const float* decoder, const p3d_render_desc* desc, const float* origin, const float* facing,
                          const uint8_t* active, const float* directions, int32_t n_directions, float ds, int32_t steps, float threshold,
                          float half_box, int32_t raster_width, uint8_t* open, uint8_t* total, p3d_stream_t stream);
int p3d_surface_shade_lit(const uint8_t* hit, const float* grad, const uint8_t* albedo, const float* cam2world, const float* light,
                          const uint8_t* ao_open, const uint8_t* ao_total, const uint8_t* sh_open, const uint8_t* sh_total, int32_t n_frames,
                          int32_t height, int32_t width, float ambient, int32_t bg_r, int32_t bg_g, int32_t bg_b, uint8_t* rgb,
                          p3d_stream_t stream);

/* ---- mesh rendering(applications/extract_mesh.py:226-262, the role of pyrender; csrc/mesh_raster.hip) ----------------------------
 * Cameras: cameras float [F][P3D_MESH_CAMERA_FLOATS], one row per frame: [0:16] cam2world row-major 4x4 in the OpenCV convention
 *   (x right, y down, z forward: columns 0..2 are the camera axes in world space, column 3 its position), [16:21] the model's
 *   parameters, [21] znear, [22] zfar with 0 < znear < zfar (so every depth is positive, as the z-test key needs), [23] unused.
 *   `orthographic` selects the model for every frame of the call:
 *     orthographic (1): xmag, ymag (pyrender's OrthographicCamera: half-extents in world units), then 3 unused floats;
 *                       u = (x_c / xmag + 1) / 2, v = (y_c / ymag + 1) / 2;
 *     pinhole      (0): fx, fy, cx, cy, skew, the normalised intrinsics of the 25-float camera label;
 *                       u = (fx x_c + skew y_c) / z_c + cx, v = fy y_c / z_c + cy  (the inverse of ray_sampler.py:43-59's lift).
 *   (x_c, y_c, z_c) = R^T (p - t) with R, t from cam2world.  Pixel (row r, col c) has its centre at u = (c + 0.5) / W,
 *   v = (r + 0.5) / H, as p3d_ray_sample's rays: a pinhole render lines up pixel for pixel with G.synthesis at the same label.
 * Projection: fp64, products summed left to right with no contraction.  Screen position in fixed point with 8 sub-pixel bits,
 *   sx = rint(u * W * 256), sy = rint(v * H * 256) (round half to even); pixel centres sit at ((c << 8) + 128, (r << 8) + 128).
 *   A vertex is DROPPED when z_c lies outside [znear, zfar] or sx / sy outside the guard band [-4096 * 256, (W or H + 4096) * 256]
 *   (or is not finite).  A triangle with a dropped vertex, or with a vertex index outside [0, V), is not drawn.  There is no
 *   clipping: a triangle that crosses znear or leaves the guard band disappears whole.
 * Coverage: edge functions E_ab(p) = (b.x - a.x)(p.y - a.y) - (b.y - a.y)(p.x - a.x) in int64 on the fixed-point coordinates.
 *   Triangles are two-sided: when E_01(v2) < 0, vertices 1 and 2 are swapped first (every later step uses that order); a triangle
 *   with E_01(v2) == 0 covers nothing.  Weights w0 = E_12(p), w1 = E_20(p), w2 = E_01(p).  A pixel centre p is covered when every
 *   w_i > 0, or w_i == 0 and the opposite edge a -> b is top-left: dy < 0, or dy == 0 and dx > 0 (y points down).  Two triangles
 *   that share an edge therefore never both cover a pixel centre on it and never both miss it.
 * Depth at a covered pixel: fp64 from the exact integer weights, in this order and with no contraction, then rounded to fp32:
 *     s = w0 + w1;  s = s + w2;
 *     orthographic: n = w0 z0;  n = n + w1 z1;  n = n + w2 z2;  depth = n / s;
 *     pinhole:      q = w0 / z0;  q = q + w1 / z1;  q = q + w2 / z2;  depth = s / q   (perspective-correct view depth).
 * Z test: key = (fp32 depth bits << 32) | face id as uint64; the smallest key wins.  A minimum does not depend on arrival order,
 *   so face id and depth are a pure function of the inputs; on equal depth the lower face id wins.  Background: face -1, depth +inf.
 * Steps of one render (all frames of the call together; F <= 65535, 1 <= W, H <= 2048, V and T <= INT32_MAX - 1):
 *   1. p3d_mesh_project: vertices float32 [V][3] -> proj int32 [F][V][4] = (sx, sy, fp32 bits of z_c, dropped 0 / 1); a dropped
 *      vertex has sx = sy = 0.
 *   2. p3d_mesh_raster_count: faces int32 [T][3] -> tile_counts int32 [F][n_tiles], n_tiles = p3d_mesh_raster_tiles(W, H) screen tiles
 *      of P3D_MESH_TILE x P3D_MESH_TILE pixels in row-major order (zeroed here): the triangles whose pixel-centre bounding box meets
 *      each tile.  The caller scans it (exclusive) into tile_offsets int64 [F][n_tiles] and copies the total to THE HOST to size the
 *      list: this sequence cannot be captured into a graph.
 *   3. p3d_mesh_raster_bin: tile_list int32 [total] <- the triangle ids of each tile, in any order inside a tile (tile_cursor int64
 *      [F][n_tiles] scratch).
 *   4. p3d_mesh_raster: one work-group per tile and frame takes the z-test minimum in an LDS buffer (64-bit LDS atomicMin) and stores
 *      face_id int32 [F][H][W] and depth float32 [F][H][W] once.
 *   5. p3d_mesh_shade: face_id, proj -> rgb uint8 [F][H][W][3].  Barycentrics from the same integer weights: orthographic w_i / s,
 *      pinhole (w_i / z_i) / q.  albedo = sum b_i colors[i] (colors uint8 [V][3], or NULL: uniform grey P3D_MESH_GREY), shaded by a
 *      headlight Lambert term albedo * (ambient + (1 - ambient) |n . f|), n the face's world normal, f the camera's forward axis
 *      (cam2world column 2); each channel rounded to nearest and clamped to 255.  Background pixels (and face ids outside [0, T))
 *      get (bg_r, bg_g, bg_b).  This is not pyrender's physically based shading.                                                    */
#define P3D_MESH_CAMERA_FLOATS 24
#define P3D_MESH_TILE 32
#define P3D_MESH_GREY 200
int p3d_mesh_project(const float* vertices, int32_t n_vertices, const float* cameras, int32_t n_frames, int32_t orthographic,
                     int32_t width, int32_t height, int32_t* proj, p3d_stream_t stream);
int32_t p3d_mesh_raster_tiles(int32_t width, int32_t height);
int p3d_mesh_raster_count(const int32_t* proj, int32_t n_vertices, const int32_t* faces, int32_t n_faces, int32_t n_frames,
                          int32_t width, int32_t height, int32_t* tile_counts, p3d_stream_t stream);
int p3d_mesh_raster_bin(const int32_t* proj, int32_t n_vertices, const int32_t* faces, int32_t n_faces, int32_t n_frames,
                        int32_t width, int32_t height, const int64_t* tile_offsets, int64_t* tile_cursor, int32_t* tile_list,
                        p3d_stream_t stream);
int p3d_mesh_raster(const int32_t* proj, int32_t n_vertices, const int32_t* faces, int32_t n_frames, int32_t width, int32_t height,
                    int32_t orthographic, const int32_t* tile_counts, const int64_t* tile_offsets, const int32_t* tile_list,
                    int32_t* face_id, float* depth, p3d_stream_t stream);
int p3d_mesh_shade(const int32_t* face_id, const int32_t* proj, const float* vertices, int32_t n_vertices, const int32_t* faces,
                   int32_t n_faces, const uint8_t* colors, const float* cameras, int32_t n_frames, int32_t orthographic, int32_t width, int32_t height,
                   float ambient, int32_t bg_r, int32_t bg_g, int32_t bg_b, uint8_t* rgb, p3d_stream_t stream);

/* ---- mesh clean-up: connected components and vertex clustering (csrc/mesh_ops.hip; pix2pix3d_amd/mesh.py) --------------------------
 * Meshes are indexed: faces int32 [T][3] into V vertices, V and T <= INT32_MAX - 1 (P3D_ERR_UNSUPPORTED beyond).  Marching cubes
 * output is welded (one vertex per crossed lattice edge), so connectivity is read off the index buffer; positions are not hashed.
 * Components: two vertices are connected when a face uses both.
 *   p3d_mesh_components: label int32 [V] <- the SMALLEST vertex id of v's connected component.  A vertex no face uses is its own
 *     component; a face with an index outside [0, V) is ignored.  Union-find: label[] starts as the identity, one thread per face
 *     hooks the larger of two roots under the smaller with a 32-bit compare-and-swap (path halving while finding), a last pass
 *     flattens every vertex to its root: three launches for any mesh.  Only roots are hooked and only under smaller ids, so each
 *     tree's root is its component's minimum whatever the order of arrival: the result is a pure function of (faces, V), the same
 *     for every face order and from run to run.  A failed compare-and-swap means another thread's hook succeeded; no thread waits
 *     for a value another thread has yet to write.
 * Vertex clustering (decimation on a regular grid of cubic cells of edge `cell` whose origin is lo, the per-axis minimum of the
 * vertices); the caller sorts and scans between the steps:
 *   1. p3d_mesh_cluster_keys: key int64 [V], key[v] = (iz * ny + iy) * nx + ix with, per axis,
 *        i = floor(((double)v - (double)lo) / (double)cell), clamped to [0, n - 1]
 *      (one IEEE fp64 subtract and one divide: a host restatement gets the same integers).  cell > 0 and finite, lo finite,
 *      nx, ny, nz >= 1 (P3D_ERR_ARGUMENT); nx * ny * nz < 2^62 (P3D_ERR_UNSUPPORTED).
 *   2. the caller sorts the vertex ids STABLY by key -> order int32 [V] (ascending vertex id inside a cell) and takes the run
 *      boundaries -> offsets int64 [C + 1] (offsets[0] = 0, offsets[C] = V); cluster c is the c-th occupied cell by ascending key.
 *      p3d_mesh_cluster_means: means float32 [C][3] <- per cluster the sum of its members in fp64, in the order of `order`, divided
 *      by their number in fp64 and rounded once to fp32.
 *   3. p3d_mesh_cluster_faces, with cluster int32 [V] the cluster of every vertex: mapped int32 [T][3] <- the face's corners as
 *      cluster ids, in the face's own order (its winding); sorted int32 [T][3] <- the same three ids ascending; degenerate uint8 [T]
 *      <- 1 when two corners share a cluster (or an index lies outside [0, V)), else 0.  The caller drops degenerate faces and,
 *      among faces with one `sorted` triple, keeps the first in input order.                                                       */
int p3d_mesh_components(const int32_t* faces, int32_t n_faces, int32_t n_vertices, int32_t* label, p3d_stream_t stream);
int p3d_mesh_cluster_keys(const float* vertices, int32_t n_vertices, float lo_x, float lo_y, float lo_z, double cell,
                          int32_t nx, int32_t ny, int32_t nz, int64_t* key, p3d_stream_t stream);
int p3d_mesh_cluster_means(const float* vertices, int32_t n_vertices, const int32_t* order, const int64_t* offsets,
                           int32_t n_clusters, float* means, p3d_stream_t stream);
int p3d_mesh_cluster_faces(const int32_t* faces, int32_t n_faces, int32_t n_vertices, const int32_t* cluster, int32_t* mapped,
                           int32_t* sorted, uint8_t* degenerate, p3d_stream_t stream);

/* ---- mesh filtering: smoothing, label voting and smooth shading over vertex adjacency (csrc/mesh_filter.hip; pix2pix3d_amd/mesh.py) ----
 * The caller builds the adjacency of the indexed mesh with sorts (mesh.adjacency): offsets int64 [V + 1] (offsets[0] = 0,
 * offsets[V] = E) and neighbours int32 [E], the list of v being neighbours[offsets[v] .. offsets[v + 1]): the distinct vertices w != v
 * that share a face with v, in ascending id.  V <= INT32_MAX - 1 (P3D_ERR_UNSUPPORTED beyond).  The kernels clamp a list to [0, E) and
 * skip an entry outside [0, V); the DEGREE of v is the number of entries that are left.  pinned uint8 [V] or NULL: a vertex with a
 * non-zero byte keeps its value.  The CPU formulation of mesh.py is the definition; the kernels' bytes equal it.
 * p3d_mesh_smooth_step: one Jacobi step of Laplacian smoothing on x float32 [V][C], 1 <= C <= 256, into out float32 [V][C], which must
 *   not overlap x (P3D_ERR_ARGUMENT).  A pinned vertex and a vertex of degree 0 copy their row bit for bit.  For every other vertex
 *   and every channel c, in fp64 with no contraction:
 *     acc = 0;  for w in list order: acc = acc + x[w][c];
 *     m = acc / degree;  d = m - x[v][c];  p = factor * d;  y = x[v][c] + p;  out[v][c] = (float)y.
 *   One thread per (vertex, channel) with the channel fastest, so that a wave reads a neighbour's row as one contiguous run; the sum
 *   runs in list order in one thread, so the output is a pure function of the inputs.  Taubin smoothing is a step with factor
 *   lambda > 0 followed by one with factor mu < -lambda, the caller alternating two buffers.
 * p3d_mesh_label_vote: one synchronous majority step on labels uint8 [V] into out uint8 [V] (no overlap), 1 <= n_labels <= 256 and
 *   every label < n_labels (the caller checks).  count[l] = the number of listed neighbours with label l, plus one if v itself has l.
 *   v keeps its label when count[its label] equals the maximum count, else it takes the smallest label that reaches the maximum.
 *   Pinned and degree-0 vertices keep theirs.  All integer: the result does not depend on any order.  One thread per vertex counts
 *   in a private column of an LDS table while its list holds at most P3D_MESH_VOTE_THREAD_DEGREE entries (three walks of the list, never
 *   degree^2 work); the longer lists of a work-group are then taken one by one by the whole group with LDS atomics on a 256-entry
 *   histogram.  One launch.
 * p3d_mesh_shade_smooth: p3d_mesh_shade with interpolated vertex normals, normals float32 [V][3] (need not be unit).  Everything up
 *   to the barycentrics b is p3d_mesh_shade's.  Then, per component in fp64, products rounded one by one and summed left to right in
 *   the weight order of the triangle setup, n = b0 n_0 + b1 n_1 + b2 n_2, and the factor is
 *   ambient + (1 - ambient) |n . f| / (|n| |f|) with p3d_mesh_shade's dot products and square roots, 0 for the fraction when the
 *   denominator is not > 0.  Albedo, rounding and background are p3d_mesh_shade's.                                                    */
#define P3D_MESH_VOTE_THREAD_DEGREE 64
int p3d_mesh_smooth_step(const float* x, int32_t n_vertices, int32_t channels, const int64_t* offsets, const int32_t* neighbours,
                         int64_t n_entries, const uint8_t* pinned, double factor, float* out, p3d_stream_t stream);
int p3d_mesh_label_vote(const uint8_t* labels, int32_t n_vertices, int32_t n_labels, const int64_t* offsets, const int32_t* neighbours,
                        int64_t n_entries, const uint8_t* pinned, uint8_t* out, p3d_stream_t stream);
int p3d_mesh_shade_smooth(const int32_t* face_id, const int32_t* proj, const float* vertices, int32_t n_vertices, const int32_t* faces,
                          int32_t n_faces, const float* normals, const uint8_t* colors, const float* cameras, int32_t n_frames,
                          int32_t orthographic, int32_t width, int32_t height, float ambient, int32_t bg_r, int32_t bg_g, int32_t bg_b,
                          uint8_t* rgb, p3d_stream_t stream);

/* ---- mesh baking: vertex normals and per-vertex colours from rendered views (csrc/mesh_bake.hip; pix2pix3d_amd/texture.py) ---------
 * One thread per vertex; every sum runs in fp64 in a fixed order and every product and sum below is rounded on its own (no
 * contraction), so the outputs are pure functions of the inputs.  The CPU formulation of pix2pix3d_amd/texture.py, written operation
 * by operation, is the definition; the kernels' bytes equal it.  sqrt below is the correctly rounded IEEE square root (the kernels
 * check the target's fp64 sqrt against an exact fma residual; torch.sqrt on the CPU is NOT correctly rounded, numpy's is).  V and T <= INT32_MAX - 1 (P3D_ERR_UNSUPPORTED beyond).
 * Vertex normals (p3d_mesh_vertex_normals):
 *   The caller lists the corners of all faces per vertex in ascending (face id, corner) order — a STABLE sort of the 3 T entries of
 *   faces by vertex id — as corner_face int32 [3 T], the face of every listed corner, and offsets int64 [V + 1] (offsets[0] = 0,
 *   offsets[V] = 3 T).  normals float32 [V][3] <- the sum over v's list, in list order, starting from 0, of
 *     cross(p1 - p0, p2 - p0), each component a * b - c * d with both products rounded,
 *   p0, p1, p2 the face's corners in fp64 (area weighting; the sign follows the faces' winding, nothing below depends on it), divided
 *   by len = sqrt(x * x + y * y + z * z) (summed left to right) and rounded to fp32.  A vertex with no faces, or with a zero or
 *   non-finite len, gets (0, 0, 0).  A face that uses a vertex twice is listed twice by it (its cross product is 0); a list entry or a
 *   face index out of range is skipped.
 * Baking (p3d_mesh_bake_accumulate, then p3d_mesh_bake_finish).  Inputs per view f and vertex v: proj int32 [F][V][4] = (sx, sy, fp32
 *   bits of z, dropped) from p3d_mesh_project; face_id int32 / depth float [F][H][W] from p3d_mesh_raster for the same mesh and
 *   cameras; images uint8 [F][H][W][3]; vertices, normals float32 [V][3]; cameras float [F][P3D_MESH_CAMERA_FLOATS] (only the pose is
 *   read).  F <= 65535, 1 <= W, H <= 2048, power in 1 .. 8, tolerance and min_cos finite and >= 0 (else P3D_ERR_ARGUMENT, before any
 *   launch).
 *   1. Texel position: tx = sx - 128, ty = sy - 128; c0 = tx >> 8, r0 = ty >> 8, fx = tx & 255, fy = ty & 255.  The footprint is
 *      pixels (r0, c0), (r0, c0 + 1), (r0 + 1, c0), (r0 + 1, c0 + 1): the four pixel centres around the vertex.
 *   2. The sample counts only if v is not dropped, the whole footprint lies inside the frame, all four face_id >= 0 (no image
 *      background bleeds in at silhouettes) and (double)z <= (double)min(depth of the four) + tolerance.
 *   3. View direction d = camera position - p (pinhole) or minus the camera's forward axis (orthographic);
 *      cos = |n . d| / (sqrt(n . n) sqrt(d . d)) in fp64, dot products summed left to right, 0 when the denominator is not > 0.  The
 *      sample counts only if cos >= min_cos.  Weight w = cos^power by repeated multiplication (w = cos; w = w * cos; ...).
 *   4. Colour per channel: ((256 - fy)(256 - fx) I00 + (256 - fy) fx I01 + fy (256 - fx) I10 + fy fx I11) / 65536, the numerator an
 *      exact integer converted to fp64.
 *   5. In view order, for every sample that counts: acc[v] += (w r, w g, w b, w) (double [V][4]) and seen[v] += 1 (int32 [V]).  acc
 *      and seen are IN/OUT: groups of views chain into exactly the sums of one call.  A frame less than 2 pixels wide or high holds
 *      no footprint: nothing is launched.
 *   6. p3d_mesh_bake_finish: colors uint8 [V][3] <- floor(acc.rgb / acc.w + 0.5) clamped to [0, 255] where acc.w > 0; elsewhere
 *      fallback[v] (uint8 [V][3]) or, with fallback NULL, (fb_r, fb_g, fb_b).                                                       */
int p3d_mesh_vertex_normals(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces,
                            const int32_t* corner_face, const int64_t* offsets, float* normals, p3d_stream_t stream);
int p3d_mesh_bake_accumulate(const int32_t* proj, const int32_t* face_id, const float* depth, const uint8_t* images,
                             const float* vertices, const float* normals, const float* cameras, int32_t n_vertices, int32_t n_frames,
                             int32_t orthographic, int32_t width, int32_t height, double tolerance, double min_cos, int32_t power,
                             double* acc, int32_t* seen, p3d_stream_t stream);
int p3d_mesh_bake_finish(const double* acc, int32_t n_vertices, const uint8_t* fallback, int32_t fb_r, int32_t fb_g, int32_t fb_b,
                         uint8_t* colors, p3d_stream_t stream);

/* ---- mesh atlas: a per-triangle texture atlas, its texels' geometry, its image and a shade that samples it (csrc/mesh_atlas.hip;
 * pix2pix3d_amd/atlas.py) ----------------------------------------------------------------------------------------------------------
 * As in "mesh baking": fp64, every product and sum rounded on its own in the stated order; the CPU formulation of atlas.py is the
 * definition and the kernels' bytes equal it (a shaded frame: within the one level of p3d_mesh_shade's headlight term).
 * Layout.  The texture is size x size texels, 16 <= size <= 8192, row 0 at the top.  Square cells of cell x cell texels, cell >= 4, lie
 *   on a grid of per_row = size / cell (integer division) cells per row in row-major order; cell k holds face 2 k (its "lower" half)
 *   and face 2 k + 1 (its "upper" half), so T faces take n_cells = (T + 1) / 2 cells, and n_cells <= per_row^2 is required
 *   (P3D_ERR_ARGUMENT; atlas.layout picks the largest cell that fits).  Inside a cell, texel (column i, row j) belongs to the lower
 *   face when i + j <= cell - 2, else to the upper face.  With m = cell - 3 the triangle's side in texels, the corners sit at the
 *   texel CENTRES (0, 0), (m, 0), (0, m) (lower, corners 0, 1, 2) and (cell - 1, cell - 1), (cell - 1 - m, cell - 1),
 *   (cell - 1, cell - 1 - m) (upper).  A texel's barycentric numerators over m are (n0, n1, n2) = (m - i' - j', i', j') with
 *   (i', j') = (i, j) (lower) or (cell - 1 - i, cell - 1 - j) (upper); n0 < 0 (one diagonal of the lower half, two of the upper) is the
 *   gutter, which takes the same formula: linear extrapolation in the triangle's plane, so that a bilinear lookup of a field that is
 *   linear over the face is exact up to the hypotenuse.  A 2 x 2 bilinear footprint at any point of a face's triangle, placed by the
 *   fixed-point rule below, puts non-zero weight only on texels that face owns: nothing bleeds between halves or cells.
 * p3d_mesh_atlas_texels: one texel per thread in cell-major order, q = (k * cell + j) * cell + i, K = n_cells * cell^2 texels.
 *   face int32 [K] <- 2 k + half, or -1 when that face does not exist (the upper half of the last cell for odd T) or one of its
 *   vertex indices lies outside [0, V); points, texel_normals float32 [K][3] <- per component, with a_c the fp64 value of vertices
 *   (or normals) float32 [V][3] at the face's corner c,
 *     s = n0 a_0;  s = s + n1 a_1;  s = s + n2 a_2;  s / m, rounded to fp32
 *   (0 where face is -1).  A texel at a corner reproduces that vertex bit for bit.  The normals are not normalised.
 * p3d_mesh_atlas_assemble: colors uint8 [K][3], face int32 [K] -> texture uint8 [size][size][3]: texel (i, j) of cell k goes to row
 *   (k / per_row) cell + j, column (k % per_row) cell + i; texels with face -1, unused cells and the right and bottom margins get
 *   (bg_r, bg_g, bg_b).  Every byte of the texture is written.
 * p3d_mesh_shade_textured: p3d_mesh_shade with the albedo taken from the texture; swap rule, barycentrics b_0..2, headlight term,
 *   rounding and background are p3d_mesh_shade's, n_faces is both the mesh's and the atlas's face count, and a face id outside
 *   [0, n_faces) is background.  The barycentrics are first put back into the face's STORED corner order (the swap rule may have
 *   exchanged corners 1 and 2).  x = b_1 m, y = b_2 m; for the upper half x = (cell - 1) - b_1 m, y = (cell - 1) - b_2 m.
 *   X = rint(x * 256), Y = rint(y * 256) (half to even), clamped to [0, (cell - 1) * 256] (a NaN to 0);
 *   c0 = min(X >> 8, cell - 2), r0 = min(Y >> 8, cell - 2), fx = X - (c0 << 8), fy = Y - (r0 << 8), both in 0 .. 256.  The four taps
 *   T00, T01, T10, T11 are the texture's texels at the cell's origin + (r0, c0), (r0, c0 + 1), (r0 + 1, c0), (r0 + 1, c0 + 1), and per
 *   channel  albedo = ((256 - fy)(256 - fx) T00 + (256 - fy) fx T01 + fy (256 - fx) T10 + fy fx T11) / 65536, the numerator an exact
 *   integer converted to fp64.  F <= 65535, 1 <= W, H <= 2048.                                                                      */
int p3d_mesh_atlas_texels(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces, const float* normals,
                          int32_t size, int32_t cell, float* points, float* texel_normals, int32_t* face, p3d_stream_t stream);
int p3d_mesh_atlas_assemble(const uint8_t* colors, const int32_t* face, int32_t n_faces, int32_t size, int32_t cell,
                            int32_t bg_r, int32_t bg_g, int32_t bg_b, uint8_t* texture, p3d_stream_t stream);
int p3d_mesh_shade_textured(const int32_t* face_id, const int32_t* proj, const float* vertices, int32_t n_vertices,
                            const int32_t* faces, int32_t n_faces, const uint8_t* texture, int32_t size, int32_t cell,
                            const float* cameras, int32_t n_frames, int32_t orthographic, int32_t width, int32_t height,
                            float ambient, int32_t bg_r, int32_t bg_g, int32_t bg_b, uint8_t* rgb, p3d_stream_t stream);

/* ---- mesh distances: surface samples, a bounding-volume hierarchy over the faces and the closest-triangle query (csrc/mesh_distance.hip;
 * pix2pix3d_amd/geometry.py) ----------------------------------------------------------------------------------------------------------
 * The kernels count in the launch counter like every mesh kernel (family 5).
 * Meshes are indexed as in "mesh clean-up" above: vertices float32 [V][3], faces int32 [T][3], V and T <= INT32_MAX - 1
 * (P3D_ERR_UNSUPPORTED beyond).  A face is VALID when its three indices lie in [0, V) and its nine coordinates are finite; every
 * kernel here skips the others.  All arithmetic below is fp64 on the fp32 inputs with one rounding per operator and no contraction
 * (#pragma clang fp contract(off), as in csrc/mesh_tri.h), so that torch's element-wise fp64 ops reproduce it bit for bit: the CPU
 * formulation of geometry.py is the definition and the kernels' bytes equal it.  For u, v in R^3:
 *     dot(u, v)   = u0 v0;  + u1 v1;  + u2 v2          (every product rounded, summed left to right)
 *     cross(u, v) = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0)      (both products rounded, then the difference)
 * and a difference of two points is taken per component in fp64 (one rounding).
 *
 * ---- surface samples ----------------------------------------------------------------------------------------------------------
 * p3d_mesh_sample_counts: k int32 [T] <- the subdivision count of every face, 0 for a face that is not valid; capped uint8 [T] <- 1
 *   where the face wanted more than k_max.  With L2 the largest of the three squared edge lengths dot(e, e), e = b - a, c - b, a - c,
 *   and s2 = spacing^2 (computed once by the caller in fp64, > 0 and finite), k is the smallest integer in [1, k_max] with
 *       (double)(k k) s2 >= L2
 *   (k k an exact integer, one rounded product), or k_max when there is none; 1 <= k_max <= P3D_MESH_SAMPLE_KMAX.  Found by bisection on
 *   the predicate, which is monotone in k: no square root decides an integer.
 * p3d_mesh_sample_points: the face contributes k^2 points, the centroids of its k^2 congruent sub-triangles.  offsets int64 [T + 1] is
 *   the exclusive sum of k^2 over the faces (the caller's cumsum; offsets[T] = N <= INT32_MAX - 1).  Point n belongs to the face f with
 *   offsets[f] <= n < offsets[f + 1]; with r = n - offsets[f]: the first k (k + 1) / 2 are the upright sub-triangles (i, j), i + j <= k - 1,
 *   i outer and j inner, both ascending, with barycentric numerators over 3 k of (n0, n1, n2) = (3 i + 1, 3 j + 1, 3 k - n0 - n1); the
 *   k (k - 1) / 2 inverted ones (i, j), i + j <= k - 2, follow in the same order with (3 i + 2, 3 j + 2, 3 k - n0 - n1).  Per component,
 *   with a_c the face's corner c:   s = n0 a_0;  s = s + n1 a_1;  s = s + n2 a_2;  s / (3 k), rounded to fp32
 *   (the arithmetic of p3d_mesh_atlas_texels).  points float32 [N][3], face int32 [N].  Two launches with the caller's scan between them.
 *
 * ---- point-to-triangle distance -----------------------------------------------------------------------------------------------
 * tri_d2(p; a, b, c), the squared distance from p to the closed triangle; total for finite inputs (a face with two equal corners is
 * its segment, with three a point), never a NaN, and every division stands behind a test that its denominator is positive:
 *     seg(p; a, b):  e = b - a;  r = p - a;  den = dot(e, e);  num = dot(r, e);  t = den > 0 ? num / den : 0;  t = min(max(t, 0), 1);
 *                    q_k = r_k - t e_k;  seg = dot(q, q)
 *     s  = min(min(seg(p; a, b), seg(p; b, c)), seg(p; c, a))
 *     e1 = b - a;  e2 = c - a;  n = cross(e1, e2);  nn = dot(n, n);  ra = p - a;  rb = p - b;  rc = p - c
 *     wc = dot(cross(e1, ra), n);  wa = dot(cross(c - b, rb), n);  wb = dot(cross(a - c, rc), n)
 *     h  = dot(ra, n);  plane = (nn > 0 and wa >= 0 and wb >= 0 and wc >= 0) ? (h h) / nn : s;  m = min(s, plane)
 *     lo_k = min(a_k, b_k, c_k);  hi_k = max(a_k, b_k, c_k);  g_k = max(max(lo_k - p_k, p_k - hi_k), 0);  box = dot(g, g)
 *     tri_d2 = max(m, box)
 *   The last line costs nothing in accuracy (the true distance to a triangle is never below the distance to its bounding box, so it
 *   only lifts an underestimate that rounding made, e.g. of the plane term of a sliver) and is what makes the tree below exact: box
 *   is the SAME expression the query evaluates for a node's box, it is monotone in lo and hi under rounding, and a node's box contains
 *   the boxes of its faces, so box(node) <= box(face) <= tri_d2(p; face) holds for the COMPUTED values, with no appeal to error bounds.
 * closest: d2[n] = the minimum of tri_d2 over the valid faces, face[n] = the smallest face id that attains it; (+inf, -1) for a point
 *   with a non-finite coordinate and for every point when no face is valid.
 *
 * ---- the hierarchy ---------------------------------------------------------------------------------------------------------------
 * p3d_mesh_bvh_keys: key int64 [n_items] <- a 63-bit Morton key.  box float32 [6] = (lo, hi) of the finite vertices, on the device (the
 *   caller's reduction).  Item t is face t (its corner sum c_k = (a_k + b_k) + c_k) or, with faces NULL, vertex t taken three times (a
 *   query point sorts like a face at that point).  Per axis x_k = floor((c_k - 3 lo_k) / (3 (hi_k - lo_k)) 2^21) clamped to
 *   [0, 2^21 - 1], 0 where the extent is not positive; bit b of x_k goes to bit 3 b + k.  An item that is not valid gets INT64_MAX.  The
 *   keys only order the items: no result depends on them.
 * The caller sorts the face ids STABLY by key -> order int32 [T].  Leaf l holds the P3D_MESH_BVH_LEAF consecutive sorted faces
 *   order[l LEAF .. (l + 1) LEAF); n_leaves = ceil(T / LEAF), padded to n_pad, the next power of two (>= 1).  The tree is the implicit
 *   complete binary tree of 2 n_pad - 1 nodes in heap order (children of i: 2 i + 1, 2 i + 2; leaf l is node n_pad - 1 + l).
 * p3d_mesh_bvh_build: tris float32 [n_leaves LEAF][12] <- per sorted slot the corners a, b, c as three float4 whose first w holds the
 *   face id as int32 bits (-1: the face is not valid, or the slot lies beyond T); nodes float32 [2 n_pad - 1][8] <- (lo.xyz, -, hi.xyz, -)
 *   per node: the min / max of fp32 values, exact and order-independent; (+inf, -inf) for a node without valid faces.  One launch for
 *   the leaves, then one per level, bottom up: no work-group reads what another wrote in the same launch, so there are no flags,
 *   counters or spins.
 * p3d_mesh_closest: one point per lane; a stack of node ids in LDS (one column per lane, depth + 1 <= 32 rows, sized by the launch).
 *   At an inner node both children's box distances are computed, the farther is pushed and the nearer entered; a node is entered or
 *   pushed only if NOT box (1 - 2^-P3D_MESH_BVH_MARGIN_LOG2) > best, and tested again when popped.  By the inequality above pruning
 *   without any margin is already exact for the computed values; the margin (2^-20, far above the 2^-52 of fp64) is kept so that
 *   the property does not hang on that argument alone.  Ties go to the smaller face id and equal box bounds are entered, so the
 *   result is the definition's, bit for bit, whatever the traversal order.  The loop visits every node at most once; it counts its
 *   iterations and, past the node count (or on a full stack), stores 1 to status int32 [1] (zeroed by the caller) and gives (+inf, -2)
 *   instead of running on: the caller reports P3D_ERR_LAUNCH.  d2 double [N], face int64 [N].
 */
#define P3D_MESH_SAMPLE_KMAX 1024
#define P3D_MESH_BVH_LEAF 4
#define P3D_MESH_BVH_MARGIN_LOG2 20
#define P3D_MESH_BVH_MAX_DEPTH 31

int p3d_mesh_sample_counts(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces, double spacing2,
                           int32_t k_max, int32_t* k, uint8_t* capped, p3d_stream_t stream);
int p3d_mesh_sample_points(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces, const int32_t* k,
                           const int64_t* offsets, int64_t n_points, float* points, int32_t* face, p3d_stream_t stream);
int p3d_mesh_bvh_keys(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_items, const float* box,
                      int64_t* key, p3d_stream_t stream);
int p3d_mesh_bvh_build(const float* vertices, int32_t n_vertices, const int32_t* faces, int32_t n_faces, const int32_t* order,
                       int32_t n_pad, float* tris, float* nodes, p3d_stream_t stream);
int p3d_mesh_closest(const float* points, int64_t n_points, const float* tris, const float* nodes, int32_t n_faces, int32_t n_pad,
                     double* d2, int64_t* face, int32_t* status, p3d_stream_t stream);

/* z_coarse [R][S_c], w_coarse [R][S_c-1], u_fine [R][S_f] -> z_fine [R][S_f] (sorted ascending
 * when `sorted`, else in draw order as sample_pdf returns them).                               */
int p3d_importance_sample(const float* z_coarse, const float* w_coarse, const float* u_fine, float* z_fine,
                          int32_t n_rays, int32_t depth_resolution, int32_t n_importance, int32_t sorted,
                          p3d_stream_t stream);

/* The same launch with the INTEGER results of the index work exposed (parity tests: bit-exact against torch.searchsorted / a stable argsort):
 *   bin_index   [R][S_f] int32, optional: per importance draw j the index torch.searchsorted(cdf, u, right=True) returns (renderer.py:240), in draw order;
 *   merge_words [R][4] uint32, optional (needs `sorted`): bit k set <=> sample k of the merged, depth-ordered ray (unify_samples, renderer.py:157-167) is an
 *               importance sample — computed by the merge step the fused ray-marcher runs (csrc/render_device.h: merge_takes_coarse).                       */
int p3d_importance_sample_index(const float* z_coarse, const float* w_coarse, const float* u_fine, float* z_fine, int32_t* bin_index, uint32_t* merge_words,
                                int32_t n_rays, int32_t depth_resolution, int32_t n_importance, int32_t sorted, p3d_stream_t stream);

/* ---- modulated convolution on the matrix cores (fp16 channels-last) --------------------------
 * Stand in for the per-layer inference chain of the StyleGAN2 synthesis layers:
 *   modulated_conv2d, fused branch      training/networks_stylegan2.py:34-69, 81-91
 *   conv2d / conv_transpose2d(stride 2) torch_utils/ops/conv2d_gradfix.py:37-45 via conv2d_resample.py:114-136
 *   noise add + bias_act epilogue       training/networks_stylegan2.py:319-332
 *   ToRGB 1x1 modulated conv            training/networks_stylegan2.py:355-359                    */

/* weight [Co][Ci][taps] fp32 (taps = kh*kw, PyTorch OIHW order), styles [N][Ci] fp32 ->
 * out (dtype fp16 or fp32) = weight * pre_scale * styles (* rsqrt(sum^2 + 1e-8) if demodulate), laid out
 * [N][Co][taps][Ci] (tap-major K, what p3d_conv2d_nhwc consumes) or, with oihw_order != 0, [N][Co][Ci][taps].   */
int p3d_modulate_weights(const float* weight, const float* styles, void* out, int dtype, int32_t n_img, int32_t co, int32_t ci,
                         int32_t taps, int32_t demodulate, float pre_scale, int32_t oihw_order, p3d_stream_t stream);

/* x [N][H][W][Ci], w [N or 1][Co][k*k][Ci] (w_img_stride elements between images, 0 = shared), both `dtype`
 * (P3D_F16: v_mfma_f32_32x32x16_f16; P3D_F32: v_mfma_f32_32x32x2_f32, exact fp32), fp32 accumulation.
 * resample = 0: k x k correlation (k = 1 or 3), "same" padding -> y [N][H][W][Co]; optional epilogue
 *   v = acc + noise[H][W] * noise_strength[0] + bias[co]; act (0 linear, 1 lrelu 0.2); * gain; clamp (< 0 off).
 * resample = 1 (k = 3): conv_transpose2d(stride 2, padding 0) -> y [N][2H+1][2W+1][Co], no epilogue.
 * resample = 2: valid (unpadded) correlation at stride 2 -> y [N][(H-k)/2+1][(W-k)/2+1][Co] with the epilogue: the strided
 * conv conv2d_resample runs after its low-pass FIR in the down-2 layers (conv2d_resample.py:108-111).
 * zeros128: >= 128 bytes of zeros in device memory, 16-byte aligned (source of the border rows of the LDS-DMA
 * staging).  Ci must be a multiple of 64 (fp16) / 32 (fp32), else P3D_ERR_UNSUPPORTED.             */
int p3d_conv2d_nhwc(const void* x, const void* w, void* y, int dtype, const float* bias, const float* noise, const float* noise_strength,
                    const void* zeros128, int32_t n_img, int32_t h, int32_t wdt, int32_t ci, int32_t co, int64_t w_img_stride,
                    int32_t kernel_size, int32_t resample, int32_t act, float gain, float clamp, p3d_stream_t stream);

/* ---- conv2d_gradfix: training-mode convolution, its data gradient and its weight gradient ---------------------------------------
 * Stand in for the vendor-library calls behind torch_utils/ops/conv2d_gradfix.py (cuDNN there, MIOpen on ROCm):
 *   forward            conv2d_gradfix.py:37-45, 107-131   F.conv2d / F.conv_transpose2d
 *   p3d_conv2d_bwd_data    :139-143   "grad_input = the transposed op" with output_padding from the shapes (:95-104)
 *   p3d_conv2d_bwd_weight  :155-194   Conv2dGradWeight (aten::convolution_backward with mask [F,T,F]; a matmul for 1x1)
 * All tensors channels-last ([N][H][W][C]), fp16 or fp32 with fp32 accumulation (dtype P3D_F32_BF16X3 for forward / bwd_data: fp32 tensors,
 * products as three bf16 MFMAs; P3D_F32_BF16X6 for all three: fp32 tensors, fp32-accurate products as six bf16 MFMAs — the weight gradient
 * takes it for whole 128 x 128 tiles and the exact kernels otherwise), groups = 1, dilation = 1, weights SHARED across the
 * batch and passed in torch's own layout and in the activation dtype.  The family (what conv2d_resample.py:96-136 ever asks for):
 *   transposed = 0: conv2d,            weight [Co][Ci][k][k]:  k in {1, 3} at stride 1 / padding k/2,  k = 3 at stride 2 / padding 0
 *   transposed = 1: conv_transpose2d,  weight [Ci][Co][k][k]:  the same two geometries; at stride 2 the output is [2H+1 | 2H+2]
 *                   (out_h / out_w; 0 = 2H+1: output_padding 0)
 * ci = channels of x, co = channels of y in every call.  w_scratch: co*ci*k*k elements of the activation dtype, 16-byte aligned (the
 * tap-major re-layout the matrix-core kernels read; unused by the skinny 1x1 route, may then be null).  zeros128 as p3d_conv2d_nhwc.
 * Returns P3D_ERR_UNSUPPORTED when ci is not a multiple of 64 (fp16) / 32 (fp32) on the 3x3 routes: pad the channels.               */
/* workspace: optional device scratch for the split-K schedule of low-resolution layers (a 512-channel 3x3 layer at 4^2 .. 32^2 is a
 * handful of output tiles with a 144-step K loop: its K steps are dealt to many work-groups and a second launch sums them);
 * p3d_conv2d_forward_workspace(...) says how many bytes a call would use (0: none), 16-byte aligned; null = never split.            */
int p3d_conv2d_forward(const void* x, const void* weight, void* y, void* w_scratch, const void* zeros128, int dtype,
                       int32_t n_img, int32_t h, int32_t w, int32_t ci, int32_t co, int32_t kernel_size, int32_t stride,
                       int32_t transposed, int32_t out_h, int32_t out_w, void* workspace, int64_t workspace_bytes, p3d_stream_t stream);
int64_t p3d_conv2d_forward_workspace(int dtype, int32_t n_img, int32_t h, int32_t w, int32_t ci, int32_t co, int32_t kernel_size, int32_t stride,
                                     int32_t transposed);
/* gy [N][gy_h][gy_w][co] -> gx [N][x_h][x_w][ci], for the FORWARD op (ci -> co, weight, kernel_size, stride, transposed) described above;
 * workspace as p3d_conv2d_forward_workspace(dtype, n_img, gy_h, gy_w, co, ci, kernel_size, stride, !transposed)                      */
int p3d_conv2d_bwd_data(const void* gy, const void* weight, void* gx, void* w_scratch, const void* zeros128, int dtype,
                        int32_t n_img, int32_t gy_h, int32_t gy_w, int32_t ci, int32_t co, int32_t kernel_size, int32_t stride,
                        int32_t transposed, int32_t x_h, int32_t x_w, void* workspace, int64_t workspace_bytes, p3d_stream_t stream);
/* gw[cs][cb][ky][kx] = sum_{n,i,j} small[n,i,j,cs] * big[n, i*stride + ky - pad, j*stride + kx - pad, cb]   (out-of-image = 0)
 * conv2d:           small = gy (cs = Co), big = x  (cb = Ci)  ->  gw [Co][Ci][k][k]
 * conv_transpose2d: small = x  (cs = Ci), big = gy (cb = Co)  ->  gw [Ci][Co][k][k]        (the roles swap, conv2d_gradfix.py:173)
 * gw in the activation dtype.  workspace: p3d_conv2d_bwd_weight_workspace(...) bytes of device scratch, 16-byte aligned (fp32
 * partial sums of the split-K work-groups; deterministic: no atomics).                                                             */
int64_t p3d_conv2d_bwd_weight_workspace(int dtype, int32_t n_img, int32_t small_h, int32_t small_w, int32_t c_small, int32_t c_big, int32_t kernel_size);
int p3d_conv2d_bwd_weight(const void* small_img, const void* big_img, void* gw, void* workspace, int64_t workspace_bytes, int dtype,
                          int32_t n_img, int32_t small_h, int32_t small_w, int32_t c_small, int32_t big_h, int32_t big_w, int32_t c_big,
                          int32_t kernel_size, int32_t stride, int32_t pad, p3d_stream_t stream);
/* The same sums, written as fp32 whatever the activation dtype and multiplied by `scale` on the way out — the gradient of a PARAMETER that entered the
 * convolution as (weight * gain).to(activation dtype) (Conv2dLayer, networks_stylegan2.py:177-180: the cast's and the gain's gradients in the final pass
 * over the partial sums instead of two more launches).  gw_f32 [cs][cb][k][k] float.                                                                  */
int p3d_conv2d_bwd_weight_scaled(const void* small_img, const void* big_img, float* gw_f32, void* workspace, int64_t workspace_bytes, int dtype,
                                 int32_t n_img, int32_t small_h, int32_t small_w, int32_t c_small, int32_t big_h, int32_t big_w, int32_t c_big,
                                 int32_t kernel_size, int32_t stride, int32_t pad, float scale, p3d_stream_t stream);

/* The kernel a p3d_conv2d_bwd_weight* call with these sizes and operand facts would run, without launching anything (read-only: tests pin the host
 * path's route decision with it).  Returns a p3d_wgrad_route code, or a negative p3d_status exactly as the call itself would for these sizes (pointer
 * checks excepted: there are no pointers here).  flags: P3D_WGRAD_* bits below — which of the two images sits on a 16-byte boundary.
 * workspace_bytes: what the call brings (< 0: as much as wanted).  plan_out (optional, 8 ints): grid, ksplit, chunks, chunks_per_split, psplit,
 * narrow_b, xcd_pad of the launch and the number of partial tiles its reduce launch sums.                                                          */
enum p3d_wgrad_route {
    P3D_WGRAD_ROUTE_SKINNY_F16    = 0,   /* skinny_wgrad_kernel<__half>: 1x1, a handful of channels on one side (memory pass)               */
    P3D_WGRAD_ROUTE_SKINNY_F32    = 1,   /* skinny_wgrad_kernel<float>                                                                       */
    P3D_WGRAD_ROUTE_TR_SMALL_ROWK = 2,   /* conv_wgrad_tr_f16_kernel<true, true>: both sides <= 64 channels, rows of 128 pixels              */
    P3D_WGRAD_ROUTE_TR_SMALL      = 3,   /* conv_wgrad_tr_f16_kernel<false, true>: both sides <= 64 channels                                 */
    P3D_WGRAD_ROUTE_TR_ROWK       = 4,   /* conv_wgrad_tr_f16_kernel<true, false>: rows of 64 pixels                                         */
    P3D_WGRAD_ROUTE_TR            = 5,   /* conv_wgrad_tr_f16_kernel<false, false>: fp16, aligned whole channel groups                       */
    P3D_WGRAD_ROUTE_F16_SMALL     = 6,   /* conv_wgrad_kernel<__half, 128, true, true>: only with P3D_WGRAD_NO_TR / _NO_TR_SMALL             */
    P3D_WGRAD_ROUTE_F16_FAST      = 7,   /* conv_wgrad_kernel<__half, 64, true>: only with P3D_WGRAD_NO_TR (/ _NO_SMALL at <= 64 channels)  */
    P3D_WGRAD_ROUTE_F16_GENERAL   = 8,   /* conv_wgrad_kernel<__half, 64, false>: any fp16 geometry                                          */
    P3D_WGRAD_ROUTE_F32_SMALL     = 9,   /* conv_wgrad_kernel<float, 32, true, true>: both sides <= 64 channels                              */
    P3D_WGRAD_ROUTE_F32_X6        = 10,  /* conv_wgrad_kernel<float, 16, true, false, true>: P3D_F32_BF16X6 on whole 128 x 128 tiles         */
    P3D_WGRAD_ROUTE_F32_FAST      = 11,  /* conv_wgrad_kernel<float, 16, true>: aligned whole channel groups                                 */
    P3D_WGRAD_ROUTE_F32_GENERAL   = 12   /* conv_wgrad_kernel<float, 16, false>: any fp32 geometry                                           */
};
enum { P3D_WGRAD_SMALL_ALIGNED = 1, P3D_WGRAD_BIG_ALIGNED = 2 };
int p3d_conv2d_bwd_weight_route(int dtype, int32_t n_img, int32_t small_h, int32_t small_w, int32_t c_small, int32_t big_h, int32_t big_w, int32_t c_big,
                                int32_t kernel_size, int32_t stride, int32_t pad, uint32_t flags, int64_t workspace_bytes, int32_t* plan_out);

/* p3d_conv2d_nhwc with optional split-K scratch (see p3d_conv2d_forward): workspace of p3d_conv2d_nhwc_workspace(...) bytes, or null */
int p3d_conv2d_nhwc_ws(const void* x, const void* w, void* y, int dtype, const float* bias, const float* noise, const float* noise_strength,
                       const void* zeros128, int32_t n_img, int32_t h, int32_t wdt, int32_t ci, int32_t co, int64_t w_img_stride,
                       int32_t kernel_size, int32_t resample, int32_t act, float gain, float clamp, void* workspace, int64_t workspace_bytes,
                       p3d_stream_t stream);
/* The last 3x3 layer of a synthesis block and its ToRGB in one launch (fp16, Co = 128 or 256: SynthesisBlock.conv1 + .torgb + the skip-image
 * sum, training/networks_stylegan2.py:449-459): y = act(conv3x3(x, w) + bias) * gain, clamped, as p3d_conv2d_nhwc would write it, and
 *   rgb_out[n][o][pixel] += clamp(sum_c y[n][pixel][c] * rgb_w[n][o][c] + rgb_bias[o], rgb_clamp)        (rgb_out fp32 NCHW, o < rgb_co <= 8)
 * from the finished tile while it is still in LDS.  rgb_w = ToRGB weight * styles, fp32 [N][rgb_co][Co].  No noise input (layers with
 * noise keep the two-launch form).  Co = 256: a work-group walks both 128-channel blocks of its pixel patch and sums the two
 * contractions before bias / clamp.  Any other Co, Ci % 64 != 0 or images under 32 x 32: P3D_ERR_UNSUPPORTED.
 * y may be NULL: the activations are then not stored at all — the LAST block of a super-resolution head returns x to a caller that drops
 * it (training/superresolution.py:297-354 return rgb only), so its 268 MB of fp16 activations per launch have the ToRGB as only reader.  */
int p3d_conv3x3_torgb_f16(const void* x, const void* w, void* y, const float* bias, const void* zeros128, const float* rgb_w, const float* rgb_bias,
                          float* rgb_out, int32_t rgb_co, float rgb_clamp, int32_t n_img, int32_t h, int32_t wdt, int32_t ci, int32_t co,
                          int64_t w_img_stride, int32_t act, float gain, float clamp, p3d_stream_t stream);

/* The LAST 3x3 layer of the tri-plane backbone and its wide ToRGB + skip-image sum in one launch (bf16x3 on split activations, Co = 128: SynthesisBlock.conv1 +
 * .torgb + the upsampled predecessor image, training/networks_stylegan2.py:449-459, for a block whose x the network drops — SynthesisNetwork.forward returns img only,
 * :511-528).  x_split / w_split as p3d_conv2d_nhwc_bf16x3_io takes them (x_split = 1); the layer's activations y = clamp(act(conv3x3 + noise + bias) * gain) are formed in
 * registers, split into (hi, lo) as their stored form would have been, and contracted with rgb_wmod_split ([N][rgb_co][1][Co] split K rows: p3d_modulate_weights,
 * P3D_F32_BF16X3, no demodulation) as p3d_torgb_wide_split does:
 *   img[n][pixel][o] = clamp(sum_c y[n][pixel][c] * rgb_w[n][o][c] + rgb_bias[o], rgb_clamp) + upsample2d(prev, f)[n][pixel][o]       (img, prev fp32 NHWC)
 * y itself is never written.  prev (and f4x4_host: sixteen HOST floats, the 4 x 4 filter) may be NULL: no skip term.  rgb_co in {32, 64, 96}; Co != 128, Ci % 32 != 0,
 * images under 32 x 32 or odd-sized, or fewer than 192 patches of 16 x 16 pixels: P3D_ERR_UNSUPPORTED (the caller keeps the two-launch form).                          */
int p3d_conv3x3_torgb_split(const void* x_split, const void* w_split, const float* bias, const float* noise, const float* noise_strength, const void* zeros128,
                            const void* rgb_wmod_split, const float* rgb_bias, float* img_nhwc, const float* prev_nhwc, const float* f4x4_host,
                            int32_t rgb_co, float rgb_clamp, int32_t n_img, int32_t h, int32_t wdt, int32_t ci, int32_t co, int64_t w_img_stride,
                            int32_t act, float gain, float clamp, p3d_stream_t stream);

/* p3d_conv2d_nhwc_ws with a per-(image, output channel) factor on the accumulator, ahead of noise / bias / activation: out_scale fp32
 * [N][Co].  With p3d_demod_coefs and p3d_bcast_fma this is the SHARED-weight form of the modulated convolution
 * (training/networks_stylegan2.py:70-79: x * styles -> convolution with the unmodulated weights -> * demodulation coefficients), which for
 * the low-resolution layers of a batch reads one weight tensor instead of one per image.  fp32 tensors (P3D_F32 / P3D_F32_BF16X3). */
int p3d_conv2d_nhwc_scaled(const void* x, const void* w, void* y, int dtype, const float* out_scale, const float* bias, const float* noise,
                           const float* noise_strength, const void* zeros128, int32_t n_img, int32_t h, int32_t wdt, int32_t ci, int32_t co,
                           int64_t w_img_stride, int32_t kernel_size, int32_t resample, int32_t act, float gain, float clamp, void* workspace,
                           int64_t workspace_bytes, p3d_stream_t stream);
/* ... and with the style modulation of that form applied on the way INTO the matrix cores: in_scale fp32 [N][Ci] multiplies every activation as it is
 * split for the MFMAs (the same fp32 product `x * styles` a separate pass would have stored: results are bit-identical to p3d_bcast_fma followed by
 * p3d_conv2d_nhwc_scaled), so the low-resolution layers lose one launch each.  dtype P3D_F32_BF16X3 only; P3D_ERR_UNSUPPORTED when the images one
 * 128-row tile touches times Ci exceed the kernel's 2048-float table (the caller then scales x itself).                                          */
int p3d_conv2d_nhwc_scaled_in(const void* x, const void* w, void* y, int dtype, const float* in_scale, const float* out_scale, const float* bias,
                              const float* noise, const float* noise_strength, const void* zeros128, int32_t n_img, int32_t h, int32_t wdt, int32_t ci,
                              int32_t co, int64_t w_img_stride, int32_t kernel_size, int32_t resample, int32_t act, float gain, float clamp,
                              void* workspace, int64_t workspace_bytes, p3d_stream_t stream);
/* Activations that stay split between the bf16x3 layers of an inference pass (training/networks_stylegan2.py:436-459: conv0 -> conv1 -> ToRGB /
 * the next block, each a modulated_conv2d :26-105 whose fp32 products this library forms as three bf16 MFMAs).  x_split != 0: x is NOT fp32 but,
 * per pixel and 32 channels, [32 x bf16 hi | 32 x bf16 lo] in the same 128 bytes (hi = bf16(v), lo = bf16(v - hi): exactly what the kernels
 * otherwise compute in registers for every tap) — as written by a call with y_split != 0 or by p3d_fir4_bias_act_nhwc_split.  The same products
 * as the plain-tensor calls: bit-identical where the same kernel runs; 3x3 'same' layers with x_split whose 16 x 16-patch grid fills the chip take a
 * ring-pipeline kernel that sums them in another order (<= 1e-6 of the range apart).  dtype is implied (P3D_F32_BF16X3: w from p3d_modulate_weights in that layout).  x_split is taken by
 * every route (3x3, 1x1, transposed, stride 2); y_split only by the 3x3 'same' layers the halo-slab / ring kernels run (Co % 32 == 0, an image of at
 * least 8 x 16 whose own grid fills the chip): otherwise P3D_ERR_UNSUPPORTED and nothing is launched — ask again with y_split = 0.           */
int p3d_conv2d_nhwc_bf16x3_io(const void* x, const void* w, void* y, const float* bias, const float* noise, const float* noise_strength,
                              const void* zeros128, int32_t n_img, int32_t h, int32_t wdt, int32_t ci, int32_t co, int64_t w_img_stride,
                              int32_t kernel_size, int32_t resample, int32_t act, float gain, float clamp, int32_t x_split, int32_t y_split,
                              void* workspace, int64_t workspace_bytes, p3d_stream_t stream);
/* The route p3d_conv2d_nhwc_bf16x3_io would take for these sizes, without launching anything: returns 1 when a split result would be granted
 * (want_y_split != 0 and the 3x3 halo-slab / ring kernel takes the layer), 0 when the result will be a plain tensor, or a negative error code;
 * *workspace_bytes = the split-K scratch that route wants (0: none).  Ask once per geometry, then call with the granted flag.                 */
int p3d_conv2d_nhwc_bf16x3_io_plan(int32_t n_img, int32_t h, int32_t wdt, int32_t ci, int32_t co, int64_t w_img_stride, int32_t kernel_size,
                                   int32_t resample, int32_t x_split, int32_t want_y_split, int64_t* workspace_bytes);
/* Wide ToRGB + skip-image sum of a synthesis block in one pass, on split activations (training/networks_stylegan2.py:355-359 ToRGBLayer and :453-459
 * img = upsample2d(img) + y):  y[n][p][o] = clamp(sum_c x[n][p][c] * wmod[n][o][c] + bias[o]) + (prev ? upfirdn2d(prev, f, up = 2, pad 2, gain 4)[n][p][o] : 0).
 * x_split [N][H][W][Ci] and wmod_split [N][Co][Ci] in the split K-row layout above (wmod: p3d_modulate_weights(..., demodulate = 0, P3D_F32_BF16X3));
 * y [N][H][W][Co] and prev [N][H/2][W/2][Co] fp32 channels-last; f4x4_host: the 16 filter taps in HOST memory, row-major (read when prev != null).
 * The skip term is summed exactly as p3d_upfirdn2d_acc sums it.  Ci in {128, 256}, Co in {32, 64, 96}, W % 32 == 0, else P3D_ERR_UNSUPPORTED.  */
int p3d_torgb_wide_split(const void* x_split, const void* wmod_split, const float* bias, float* y_nhwc, const float* prev_nhwc, const float* f4x4_host,
                         int32_t n_img, int32_t h, int32_t w, int32_t ci, int32_t co, float clamp, p3d_stream_t stream);
/* d[n][o] = rsqrt(sum_i styles[n][i]^2 * w2[o][i] + 1e-8) with w2[o][i] = sum over the taps of weight[o][i][.]^2 (networks_stylegan2.py:57-63) */
int p3d_demod_coefs(const float* styles, const float* w2, float* d, int32_t n_rows, int32_t ci, int32_t co, p3d_stream_t stream);
/* Several layers at once (one launch): job j writes d_j [n_rows][co_j] from styles_j [n_rows][ci_j] and w2_j [co_j][ci_j]; all jobs share n_rows.  The
 * job array is HOST memory, copied into the kernel arguments.  Results are bit-identical to p3d_demod_coefs per job.                          */
#define P3D_DEMOD_MAX_JOBS 24
typedef struct p3d_demod_job { const float* styles; const float* w2; float* d; int32_t ci, co; } p3d_demod_job;
int p3d_demod_coefs_multi(const p3d_demod_job* jobs_host, int32_t n_jobs, int32_t n_rows, p3d_stream_t stream);
/* Its gradient for the training passes: given gd = dL/dd [N][Co] and the forward's d, writes gs = dL/dstyles [N][Ci] and gw = dL/dweight [Co][Ci][taps]
 * (weight: the fp32 [Co][Ci][taps] tensor w2 was summed from); either output may be null.  The reference gets these from autograd through
 * (w * s).square().sum().rsqrt() on the [N][Co][Ci][k][k] product (networks_stylegan2.py:57-63).                                                    */
int p3d_demod_coefs_backward(const float* gd, const float* d, const float* styles, const float* w2, const float* weight, float* gs, float* gw,
                             int32_t n_rows, int32_t ci, int32_t co, int32_t taps, p3d_stream_t stream);

int64_t p3d_conv2d_nhwc_workspace(int dtype, int32_t n_img, int32_t h, int32_t wdt, int32_t ci, int32_t co, int64_t w_img_stride, int32_t kernel_size,
                                  int32_t resample);

/* The kernel family a p3d_conv2d_nhwc* call with these sizes and operand facts would run, without launching anything (read-only: tests pin the
 * host path's route decision with it).  Returns a p3d_conv_route code, or a negative p3d_status exactly as the call itself would for these sizes
 * (pointer checks excepted: there are no pointers here); *scratch_bytes (optional) = the split-K scratch that route would like, granted or not.
 * flags: P3D_CONV_* bits below — which per-image scales the call brings, whether it brings a workspace (taken to be aligned and as large as
 * wanted), whether y is 16-byte aligned.  x_split / y_split: as p3d_conv2d_nhwc_bf16x3_io.                                                    */
enum p3d_conv_route {
    P3D_CONV_ROUTE_GENERIC        = 0,   /* conv2d_nhwc_kernel: any size, any resample mode, the per-image scales                            */
    P3D_CONV_ROUTE_GENERIC_SPLITK = 1,   /* ... with its K loop dealt out over the workspace, + splitk_epilogue_kernel (two launches)        */
    P3D_CONV_ROUTE_HALO           = 2,   /* conv3x3_halo_kernel: 3x3 "same" on 8 x 16 pixel slabs                                            */
    P3D_CONV_ROUTE_HALO_X6P       = 3,   /* conv3x3_halo_x6p_kernel: the same for bf16x6 with operands split once per work-group             */
    P3D_CONV_ROUTE_H2_F16         = 4,   /* conv3x3_h2_f16_kernel: fp16 3x3 "same" on 16 x 16 patches                                        */
    P3D_CONV_ROUTE_R2_BF16X3      = 5,   /* conv3x3_r2_bf16x3_kernel: bf16x3 3x3 "same" on split activations                                 */
    P3D_CONV_ROUTE_CONVT_H2_F16   = 6    /* convT_h2_f16_kernel: fp16 transposed stride-2 form                                               */
};
enum { P3D_CONV_HAS_OUT_SCALE = 1, P3D_CONV_HAS_IN_SCALE = 2, P3D_CONV_HAS_WORKSPACE = 4, P3D_CONV_Y_ALIGNED = 8 };
int p3d_conv2d_nhwc_route(int dtype, int32_t n_img, int32_t h, int32_t wdt, int32_t ci, int32_t co, int64_t w_img_stride, int32_t kernel_size,
                          int32_t resample, int32_t x_split, int32_t y_split, uint32_t flags, int64_t* scratch_bytes);

/* x [N][HW][Ci] fp16 channels-last, weight [Co][Ci] fp32, styles [N][Ci] fp32 (weight gain already applied),
 * bias [Co] or null -> y [N][Co][HW] fp32 (NCHW); accumulate != 0 adds into y (the skip-image sum).
 * Ci in {64, 128, 256}, Co <= 32, HW a multiple of 4, else P3D_ERR_UNSUPPORTED (wide outputs: p3d_conv2d_nhwc, k = 1). */
int p3d_torgb_nhwc_f16(const void* x, const float* weight, const float* styles, const float* bias, float* y_nchw,
                       int32_t n_img, int32_t hw, int32_t ci, int32_t co, float clamp, int32_t accumulate, p3d_stream_t stream);

/* ---- per-(image, channel) scaling and its gradient reductions ----------------------------------
 * The element-wise half of the unfused modulated convolution of the training passes (training/networks_stylegan2.py:70-79:
 * x * styles before the convolution, fma(y, dcoefs, noise) after it; torch_utils/ops/fma.py:17-60) and the bias-gradient sums of
 * bias_act (bias_act.py:190-193).  A dense activation tensor is passed as [n][a][b], b contiguous: NCHW -> channels_last = 0, a = C,
 * b = H*W; channels-last -> channels_last = 1, a = H*W, b = C.  dtype fp16 or fp32, fp32 arithmetic, one rounding; b must be a multiple
 * of 8 (fp16) / 4 (fp32) else P3D_ERR_UNSUPPORTED.
 *   p3d_bcast_fma:    y = x * scale[n][c] + z[z_per_image ? n : 0][pixel]      scale fp32 [n][C]; z in x's dtype, [1 or n][H*W], or null
 *   p3d_channel_dot:  out[n][c] = sum over the pixels of p * q  (q null: of p)  fp32 out; channels-last needs a workspace of
 *                     p3d_channel_dot_workspace(...) bytes (partial sums of 256-row chunks; deterministic, no atomics)
 *   p3d_pixel_sum:    out[n][pixel] = sum over the channels of p               fp32 out                                          */
int p3d_bcast_fma(const void* x, const float* scale, const void* z, void* y, int dtype, int32_t channels_last, int32_t n, int32_t a, int32_t b,
                  int32_t z_per_image, p3d_stream_t stream);
int64_t p3d_channel_dot_workspace(int32_t channels_last, int32_t n, int32_t a, int32_t b);
int p3d_channel_dot(const void* p, const void* q, float* out, void* workspace, int64_t workspace_bytes, int dtype, int32_t channels_last,
                    int32_t n, int32_t a, int32_t b, p3d_stream_t stream);
int p3d_pixel_sum(const void* p, float* out, int dtype, int32_t channels_last, int32_t n, int32_t a, int32_t b, p3d_stream_t stream);

/* ---- the x2 synthesis layer in one launch (fp16) -----------------------------------------------
 * conv_transpose2d(stride 2, 3x3; torch_utils/ops/conv2d_resample.py:114-127) -> 4x4 low-pass, pad 1 (:128) -> + noise -> + bias ->
 * lrelu(0.2) * act_gain -> clamp (training/networks_stylegan2.py:319-332), i.e. p3d_conv2d_nhwc(resample = 1) followed by
 * p3d_fir4_bias_act_nhwc without the [N][2H+1][2W+1][Co] intermediate in memory.  x [N][H][W][Ci] fp16, w [N or 1][Co][9][Ci] fp16
 * (as for p3d_conv2d_nhwc), y [N][2H][2W][Co] fp16.  fir_yx_host: EIGHT floats in HOST memory, fy[0..3] then fx[0..3], the separable
 * filter in correlation order with its gain folded in: out[oy][ox] = sum fy[a] fx[b] ct[oy - 1 + a][ox - 1 + b].  conv_gain scales the
 * transposed conv's output before it is rounded to fp16.  act: 0 linear, 1 lrelu(0.2); bias / noise may be null; clamp < 0 = off.
 * Ci and Co must be multiples of 32, else P3D_ERR_UNSUPPORTED (callers then use the two-launch form).                       */
int p3d_up2_fir_f16(const void* x, const void* w, void* y, const void* zeros128, const float* bias, const float* noise,
                    const float* noise_strength, const float* fir_yx_host, int32_t n_img, int32_t h, int32_t wdt, int32_t ci, int32_t co,
                    int64_t w_img_stride, float conv_gain, int32_t act, float act_gain, float clamp, p3d_stream_t stream);
/* The same layer for fp32 tensors in the bf16x3 formulation (P3D_F32_BF16X3): w = p3d_modulate_weights(..., dtype P3D_F32_BF16X3)
 * [N or 1][Co][9][Ci] in its [32 x hi | 32 x lo] K rows, x / y fp32.  Arguments as p3d_up2_fir_f16.                        */
int p3d_up2_fir_bf16x3(const void* x, const void* w, void* y, const void* zeros128, const float* bias, const float* noise,
                       const float* noise_strength, const float* fir_yx_host, int32_t n_img, int32_t h, int32_t wdt, int32_t ci, int32_t co,
                       int64_t w_img_stride, float conv_gain, int32_t act, float act_gain, float clamp, p3d_stream_t stream);

/* ---- 4x4 FIR + layer epilogue, channels-last --------------------------------------------------
 * The tail of every x2 synthesis layer in one pass: upfirdn2d(up = down = 1, 4x4 filter f [4][4] fp32 contiguous,
 * gain) (torch_utils/ops/conv2d_resample.py:128) followed by "+ noise" and bias_act (networks_stylegan2.py:319-332):
 *   y = clamp(act(fir(x) + noise[out_h][out_w] * noise_strength[0] + bias[c]) * act_gain)
 * x [N][in_h][in_w][C] -> y [N][out_h][out_w][C], dtype fp16 or fp32, out = in + pad0 + pad1 - 3 (pad1 implied by the
 * sizes).  act: 1 linear, 3 lrelu(alpha) (bias_act.py:23-33 indices); bias / noise may be null; clamp < 0 = off.
 * C must be a multiple of 64 (fp16) / 32 (fp32), else P3D_ERR_UNSUPPORTED.                              */
int p3d_fir4_bias_act_nhwc(const void* x, const float* f, void* y, int dtype, int32_t n_img, int32_t c, int32_t in_h, int32_t in_w,
                           int32_t pad_x0, int32_t pad_y0, int32_t out_h, int32_t out_w, int32_t flip, float gain,
                           const float* bias, const float* noise, const float* noise_strength, int32_t act, float alpha, float act_gain,
                           float clamp, p3d_stream_t stream);
/* The same pass on fp32 input with the result written in the split layout of p3d_conv2d_nhwc_bf16x3_io (C % 32 == 0): the x2 layer's output goes
 * to the block's next bf16x3 convolution without an fp32 copy of it ever existing.                                                        */
int p3d_fir4_bias_act_nhwc_split(const void* x, const float* f, void* y, int32_t n_img, int32_t c, int32_t in_h, int32_t in_w,
                                 int32_t pad_x0, int32_t pad_y0, int32_t out_h, int32_t out_w, int32_t flip, float gain,
                                 const float* bias, const float* noise, const float* noise_strength, int32_t act, float alpha, float act_gain,
                                 float clamp, p3d_stream_t stream);

/* ---- low-resolution layers and style affines: launch-count diet (csrc/small_ops.hip) -----------
 * p3d_fc_forward: FullyConnectedLayer.forward (training/networks_stylegan2.py:113-127) in one launch:
 *   y[n][o] = act((sum_i x[n][i] * w[o][i]) * weight_gain + b[o] * bias_gain) * act_gain * out_scale
 * x [n_rows][in] (n_rows <= 16, rows x_row_stride elements apart: a column of the ws tensor is read in place), w [out][in],
 * b [out] or null, fp32; act 1 = linear, 3 = lrelu(alpha).
 * out_scale carries a constant the caller multiplies the result by (ToRGBLayer's weight_gain, :356).
 *
 * p3d_im2col3x3: the 3x3 patch matrix of the whole batch,
 *   cols[n][c * 9 + ky * 3 + kx][oy * ow + ox] = x[n, c, oy * stride + ky - pad, ox * stride + kx - pad] (0 outside),
 * oh = (h + 2 pad - 3) / stride + 1.  pad 1 / stride 1 = torch.nn.functional.unfold(x, 3, padding=1); pad 0 / stride 2 feeds the
 * valid stride-2 conv of the down-2 layers (conv2d_resample.py:108-111).  x fp32 addressed by ELEMENT strides (NCHW or
 * channels-last storage), cols fp32 contiguous.
 *
 * p3d_noise_bias_act: the tail of SynthesisLayer.forward after the convolution (:326-332) on y [n_img][c][hw] fp32:
 *   y = clamp(act(x + noise[hw] * noise_strength[0] + bias[c]) * gain);  hw % 4 == 0; x may equal y; noise / bias may be null. */
int p3d_fc_forward(const float* x, const float* w, const float* b, float* y, int32_t n_rows, int32_t in_features, int32_t out_features,
                   int64_t x_row_stride, float weight_gain, float bias_gain, int32_t act, float alpha, float act_gain, float out_scale, p3d_stream_t stream);

/* Several FullyConnectedLayer evaluations on the same number of rows in ONE launch (the style affines of a synthesis network:
 * SynthesisLayer.affine / ToRGBLayer.affine, training/networks_stylegan2.py:305, 352): jobs_host is a HOST array, its contents travel in
 * the kernel arguments.  Each job is p3d_fc_forward's argument list.  At most P3D_FC_MAX_JOBS jobs.                                  */
#define P3D_FC_MAX_JOBS 40
typedef struct p3d_fc_job {
    const float* x; const float* w; const float* b; float* y;
    int64_t x_row_stride;
    int32_t in_features, out_features;
    float weight_gain, bias_gain;
    int32_t act; float alpha, act_gain, out_scale;
} p3d_fc_job;
int p3d_fc_multi(const p3d_fc_job* jobs_host, int32_t n_jobs, int32_t n_rows, p3d_stream_t stream);
int p3d_im2col3x3(const float* x, float* cols, int32_t n_img, int32_t c, int32_t h, int32_t w, int32_t pad, int32_t stride,
                  int64_t stride_n, int64_t stride_c, int64_t stride_y, int64_t stride_x, p3d_stream_t stream);
int p3d_noise_bias_act(const float* x, float* y, const float* noise, const float* noise_strength, const float* bias, int32_t n_img,
                       int32_t c, int32_t hw, int32_t act, float alpha, float gain, float clamp, p3d_stream_t stream);

/* RaySampler.forward (training/volumetric_rendering/ray_sampler.py:24-62) in one launch: cam2world [n_cam][4][4], intrinsics
 * [n_cam][3][3] (normalised fx, fy, cx, cy, skew), fp32 contiguous -> origins, dirs [n_cam][R*R][3] fp32, rays row-major,
 * directions unit length (norm clamped at 1e-12 like F.normalize).                                                        */
int p3d_ray_sample(const float* cam2world, const float* intrinsics, float* origins, float* dirs, int32_t n_cam, int32_t resolution,
                   p3d_stream_t stream);
/* The same straight from the 25-float camera labels the generators take (training/triplane.py:57-60: c[:, :16] is cam2world, c[:, 16:25] the
 * intrinsics): labels [n_cam][label_stride] fp32, label_stride >= 25 floats between rows — no contiguous copies of the two slices.       */
int p3d_ray_sample_labels(const float* labels, int64_t label_stride, float* origins, float* dirs, int32_t n_cam, int32_t resolution, p3d_stream_t stream);

/* Displayable uint8 frames from the float outputs of a chunk of views, in ONE launch (csrc/frame_ops.hip) — the host-side finishing of the reference's
 * scripts: (clip(x, -1, 1) + 1) * 127.5 -> uint8 (applications/generate_video.py:65, 81-82; generate_samples.py:116-120) and
 * color_mask(argmax(semantic)) (generate_video.py:67; training/utils.py:5-15).  jobs_host is a HOST array of at most P3D_FRAME_MAX_JOBS jobs whose
 * contents travel in the kernel arguments (no device allocation; graph-capturable), so image + label map (+ depth) of a chunk are one launch.
 *
 * Per job: src is fp32 [n][c][h][w] addressed by the four ELEMENT strides src_stride = (n, c, y, x) — planar, channels-last or any view of either.
 * dst is uint8 with dst_bpp (1 or 3) bytes per pixel: pixel (i, y, x) of the job lands at dst + i * dst_frame_pitch + (y0 + y) * dst_row_pitch
 * + (x0 + x) * dst_bpp (pitches in BYTES), so a chunk can be written into a slice of [F][H][W][3], one half of a side-by-side video or a tile of a
 * canvas; bytes outside the rectangle are not touched.  The rectangle must lie inside its pitches.
 *   mode P3D_FRAME_SCALE (c = 1 or 3, dst_bpp = c): u8 = (uint8)clamp((x - lo) * scale, 0, 255), fp32, difference and product rounded separately,
 *     truncation toward zero, NaN -> 0; the caller passes scale = 255 / (hi - lo) rounded once (lo = -1, scale = 127.5 for images).
 *   mode P3D_FRAME_LABEL (2 <= c <= 64, dst_bpp = 3): k = argmax over the channels by torch.argmax's CPU rules (the first maximal channel wins a
 *     tie; a NaN counts as the maximum, the first NaN wins); dst gets palette[k] (uint8 [c][3]: `palette` by value, or palette_dev on the device
 *     when non-null) and, when dst_index is non-null, k itself goes as one byte per pixel to dst_index (same origin, its own pitches).            */
#define P3D_FRAME_MAX_JOBS 4
#define P3D_FRAME_SCALE 0
#define P3D_FRAME_LABEL 1
typedef struct p3d_frame_job {
    const float* src; int64_t src_stride[4];
    uint8_t* dst; int64_t dst_row_pitch, dst_frame_pitch;
    uint8_t* dst_index; int64_t index_row_pitch, index_frame_pitch;
    const uint8_t* palette_dev;
    int32_t mode, n, c, h, w, x0, y0, dst_bpp;
    float lo, scale;
    uint8_t palette[192];
} p3d_frame_job;
int p3d_frame_finish(const p3d_frame_job* jobs_host, int32_t n_jobs, p3d_stream_t stream);

/* ---- edit sessions (csrc/edit_ops.hip; pix2pix3d_amd/edit.py) -----------------------------------
 * p3d_paint_strokes: every brush stroke of a session into a uint8 label map in ONE launch — the demo's make_mask, a cv2.line per stroke over a
 * numpy mask followed by a host-to-device copy (applications/demo/qt_demo_seg2cat.py:459-463, called for every label at :432-433).
 *   base    uint8 [h][w], rows base_row_pitch bytes apart; dst the same with its own pitch, a different buffer: every pixel of dst is written
 *           exactly once, with the base value or the label of the LAST stroke in table order that covers it (= painting the strokes in order).
 *   strokes int32 [n_strokes][6] = (x0, y0, x1, y1, thickness, label) on the device, contiguous; n_strokes = 0 copies base.
 * Coverage is defined in integers (cv2's polygon fill is not specified): with d = b - a, p = pixel - a, L = d.d, s = p.d and t the thickness,
 *   s <= 0: 4 |p|^2 <= t^2;   s >= L: 4 |p - d|^2 <= t^2;   otherwise: 4 (p x d)^2 <= t^2 L
 * — the capsule of radius t / 2 about the segment; a zero-length stroke is a disc.  The caller keeps 1 <= t <= 255, 0 <= label <= 255 and the
 * endpoints in [P3D_PAINT_MIN_COORD, P3D_PAINT_MAX_COORD] (the table is device memory: pix2pix3d_amd/edit.py checks them on the host); with
 * h, w <= P3D_PAINT_MAX_SIZE these keep 4 (p x d)^2 below 2^60.  Values outside them cannot make the kernel leave the mask.
 *
 * p3d_label_features: a uint8 label map straight to the activations of the Encoder's first layer.  For a one-hot image b{res}.fromrgb (1x1
 * convolution, bias, lrelu; training/networks_stylegan2.py DiscriminatorBlock) is a lookup, out[i, :, y, x] = table[min(mask[i, y, x], n_labels)]:
 *   mask  uint8 [n][h][w], frames / rows mask_frame_pitch / mask_row_pitch bytes apart;
 *   table fp32 [n_labels + 1][c] contiguous on the device: row k the layer's output for label k, row n_labels its output for an all-zero pixel
 *         (what every byte >= n_labels reads); c % 4 == 0, 1 <= n_labels <= 255, (n_labels + 1) * (c + 4) + 4 c floats within 64 KB;
 *   out   [n][c][h][w] fp32 (P3D_F32) or fp16 (P3D_F16, round to nearest even) through the four ELEMENT strides out_stride = (n, c, y, x):
 *         16-byte stores along c (channels-last) or x (planar) where pointer and strides allow, single elements otherwise.                      */
#define P3D_PAINT_MAX_SIZE 4096
#define P3D_PAINT_MAX_STROKES 65535
#define P3D_PAINT_MIN_COORD (-4096)
#define P3D_PAINT_MAX_COORD 8191
int p3d_paint_strokes(const uint8_t* base, int64_t base_row_pitch, uint8_t* dst, int64_t dst_row_pitch, int32_t h, int32_t w,
                      const int32_t* strokes, int32_t n_strokes, p3d_stream_t stream);
int p3d_label_features(const uint8_t* mask, int64_t mask_frame_pitch, int64_t mask_row_pitch, const float* table, int32_t n_labels,
                       void* out, int32_t dtype, const int64_t* out_stride, int32_t n, int32_t c, int32_t h, int32_t w, p3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* P3D_HIP_H */
