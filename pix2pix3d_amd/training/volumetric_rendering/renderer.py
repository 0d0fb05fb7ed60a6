"""Tri-plane importance renderer.

Host-side mirror of training/volumetric_rendering/renderer.py:88-253 (``ImportanceRenderer``): same
constructor, ``forward(planes, decoder, ray_origins, ray_directions, rendering_options)`` and
``run_model(...)`` signatures, same ``rendering_options`` keys, same RNG draws in the same order.

Device tensors run ONE fused HIP kernel (csrc/render.hip through ``p3d_render_forward`` /
``p3d_sample_points``); graphs that need gradients get the same forward and a fused backward
(csrc/render_bwd.hip through ``p3d_render_backward``, see ``_FusedRenderFn``).  CPU tensors run the
tensor-op restatement below (``_forward_tensor_ops``), which is also what the reference does on every
device.  ``fused_policy = 'require'`` turns any silent use of the tensor-op path on a device tensor
into an error.
"""
import ctypes
import os
from typing import NamedTuple, Optional

import torch

from ... import _lib
from ...torch_utils.ops import modconv
from . import math_utils
from .ray_marcher import MipRayMarcher2

fused_policy = 'auto'          # 'auto' | 'require' | 'never'
_warned_routes = set()


def _tensor_op_guard(who, on_device, reason, required='fused HIP path required but unavailable', instead='the tensor-op renderer, not the fused HIP kernel'):
    """Device tensors are about to leave the native route for ``reason``: nothing under ``fused_policy = 'never'`` (and for CPU tensors), an error under
    'require', else one warning per (who, reason) — a silent fallback would look like the native path in every output but the profile.  (Expected cases: a
    gradient w.r.t. rays, depth or point coordinates, density_noise > 0, sample counts outside 4..64 coarse / 1..64 fine, a decoder that is not the OSG
    32-64-33 MLP.)  ``shape.sigma_grid`` passes its own two texts."""
    if not on_device or fused_policy == 'never':
        return
    if fused_policy == 'require':
        raise RuntimeError(f'{who}: {required}: {reason}')
    if (who, reason) not in _warned_routes:
        _warned_routes.add((who, reason))
        import warnings
        warnings.warn(f'{who}: device tensors on {instead}: {reason}', RuntimeWarning, stacklevel=3)


fused_training = True          # graphs that need gradients: fused forward + recompute-in-backward (see _FusedRenderFn)
fused_backward = True          # ... with the backward on the device kernels of csrc/render_bwd.hip (False: replay the tensor-op renderer)
mlp_bf16x3 = os.environ.get('P3D_MLP_BF16X3', '1') != '0'      # inference: the decoder MLPs as three bf16 MFMAs per fp32 product (csrc/render_device.h)
mlp_l1x6 = os.environ.get('P3D_MLP_L1X6', '1') != '0'          # exact forward passes (training, bf16x3 off), with modconv.f32_x6: layer 1 of the decoder MLPs as bf16x6 (fp32-accurate)
_RenderDesc = _lib.p3d_render_desc      # the struct class, derived from include/p3d_hip.h


def generate_planes():
    """Axes of the three feature planes (renderer.py:23-37): rows of each 3x3 are the plane's basis vectors."""
    return torch.tensor([[[1, 0, 0], [0, 1, 0], [0, 0, 1]],
                         [[1, 0, 0], [0, 0, 1], [0, 1, 0]],
                         [[0, 0, 1], [1, 0, 0], [0, 1, 0]]], dtype=torch.float32)


def project_onto_planes(planes, coordinates):
    """coordinates [N,M,3] -> in-plane (u, v) per plane, [N*n_planes, M, 2] (renderer.py:39-53)."""
    n, m, _ = coordinates.shape
    k = planes.shape[0]
    inv = torch.linalg.inv(planes)                                     # [k,3,3]
    uvw = torch.einsum('nmc,kcd->nkmd', coordinates, inv)              # row vector times inverse basis
    return uvw.reshape(n * k, m, 3)[..., :2]


def sample_from_planes(plane_axes, plane_features, coordinates, mode='bilinear', padding_mode='zeros', box_warp=None):
    """Bilinear taps of every plane at the projected points: [N, n_planes, M, C] (renderer.py:55-65)."""
    assert padding_mode == 'zeros'
    n, k, c, h, w = plane_features.shape
    m = coordinates.shape[1]
    uv = project_onto_planes(plane_axes, (2 / box_warp) * coordinates).unsqueeze(1)
    out = torch.nn.functional.grid_sample(plane_features.reshape(n * k, c, h, w), uv.float(), mode=mode,
                                          padding_mode=padding_mode, align_corners=False)
    return out.permute(0, 3, 2, 1).reshape(n, k, m, c)


def sample_from_3dgrid(grid, coordinates):
    """Trilinear lookup in a dense feature volume (renderer.py:67-80; not called by any generator, kept for the module's surface):
    grid [1 or N, C, H, W, D], coordinates [N, P, 3] in [-1, 1] -> [N, P, C]."""
    n, _, dims = coordinates.shape
    out = torch.nn.functional.grid_sample(grid.expand(n, -1, -1, -1, -1), coordinates.reshape(n, 1, 1, -1, dims),
                                          mode='bilinear', padding_mode='zeros', align_corners=False)
    n, c, h, w, d = out.shape
    return out.permute(0, 4, 3, 2, 1).reshape(n, h * w * d, c)


def _osg_mlp_layers(seq, n_in):
    """(fc1, fc2, lr_mul) of the MLP the kernels implement — FC(n_in, 64) - Softplus(1, 20) - FC(64, 33), linear, biased, gains consistent with one
    lr_mul — else None."""
    if not (isinstance(seq, torch.nn.Sequential) and len(seq) == 3 and isinstance(seq[1], torch.nn.Softplus)):
        return None
    fc1, fc2 = seq[0], seq[2]
    if not all(hasattr(fc, 'weight_gain') and hasattr(fc, 'bias_gain') and getattr(fc, 'activation', None) == 'linear' and fc.bias is not None for fc in (fc1, fc2)):
        return None
    if tuple(fc1.weight.shape) != (64, n_in) or tuple(fc2.weight.shape) != (33, 64) or seq[1].beta != 1 or seq[1].threshold != 20:
        return None
    lr = float(fc1.bias_gain)
    if abs(fc1.weight_gain - lr / n_in ** 0.5) > 1e-12 or abs(fc2.weight_gain - lr / 64 ** 0.5) > 1e-12 or fc2.bias_gain != lr:
        return None
    return fc1, fc2, lr


def _decoder_nets(decoder):
    """Recognise the OSG decoders the fused kernel implements; returns (nets, lr_mul-free raw params, sigmoid flag) or None.

    OSGDecoder (training/triplane.py:112-135): one 32->64->33 MLP.  OSGDecoder_semantic_lateSeparate
    (training/triplane_cond.py:926-970): colour net + label net, density from the label net."""
    found = [_osg_mlp_layers(getattr(decoder, name), 32) for name in ('net', 'net_semantic') if getattr(decoder, name, None) is not None]
    if len(found) not in (1, 2) or None in found or any(lr != found[0][2] for _, _, lr in found):
        return None
    if len(found) == 2 and not hasattr(decoder, 'semantic_sigmoid'):
        return None
    if len(found) == 1 and type(decoder).__name__ != 'OSGDecoder':
        return None                                  # e.g. OSGDecoder_semantic slices its outputs differently
    return [net[:2] for net in found], found[0][2], bool(getattr(decoder, 'semantic_sigmoid', False))


def _dual_decoder_nets(decoder_texture, decoder_semantic):
    """``_decoder_nets`` for the two-plane-set kernels: OSGDecoder(64) on cat(texture, semantic) + OSGDecoder_semantic(32), one lr_mul."""
    if type(decoder_texture).__name__ != 'OSGDecoder' or not hasattr(decoder_semantic, 'final_sigmoid') or hasattr(decoder_texture, 'net_semantic') \
            or hasattr(decoder_semantic, 'net_semantic'):
        return None
    tex, sem = _osg_mlp_layers(getattr(decoder_texture, 'net', None), 64), _osg_mlp_layers(getattr(decoder_semantic, 'net', None), 32)
    if tex is None or sem is None or tex[2] != sem[2]:
        return None
    return [tex[:2], sem[:2]], tex[2], bool(decoder_semantic.final_sigmoid)


def _f32c(t):
    """fp32, dense and 16-byte aligned, copied only when it is not (rays cut out of one [N, M, 6] tensor, ``expand``ed uniforms, decoder parameters that are
    views into a flat buffer: ``contiguous()`` alone hands a dense view at an odd offset on as it is)."""
    return modconv.kernel_operand(t.detach().to(torch.float32))


def shared_planes(n_planes, n_rays, who, allowed=True):
    """One plane set for every camera?  Planes of batch 1 serve ray batches of any size (a video: one latent, B views per launch); equal batches are the
    ordinary case; anything else is an error on every route, before any launch.  (``allowed=False``: the two-plane-set kernel has no shared-plane form.)"""
    if n_planes == n_rays:
        return False
    if n_planes != 1 or not allowed:
        raise ValueError(f'{who}: planes of batch {n_planes} cannot serve rays of batch {n_rays} (the batches must be equal' + (', or the planes of batch 1)' if allowed else ')'))
    return True


# ---- the route decision ---------------------------------------------------------------------------------------------------------
def fallback_reason(policy, on_device, options, decoders, graph=False, plane_shapes=None, clamp_mode=True, own=()):
    """Why a call cannot take its device kernel — the first failing condition, in the one order every entry point reports them — or None.  ``decoders``: the
    one decoder, or the (texture, semantic) pair of the two-plane-set renderer; ``graph``: an autograd graph is needed that the entry point cannot give;
    ``own``: (failed, text) conditions of the caller's, after the plane shapes (``shape.sigma_grid``)."""
    dual = len(decoders) == 2
    if policy == 'never':
        return 'fused_policy == never'
    if not on_device:
        return 'CPU tensors'
    if graph:
        return 'autograd graph requested (no fused backward for this entry point, or fused_training is off)'
    if plane_shapes is not None and (len(set(map(tuple, plane_shapes))) != 1 or len(plane_shapes[0]) != 5 or tuple(plane_shapes[0][1:3]) != (3, 32)):
        return f"planes of shape {' / '.join(str(tuple(s)) for s in plane_shapes)} are not [N,3,32,H,W]" + (' sets of one shape' if dual else '')
    for failed, text in own:
        if failed:
            return text
    if options.get('density_noise', 0) > 0:
        return 'density_noise > 0'
    if clamp_mode and options.get('clamp_mode', 'softplus') != 'softplus':
        return "clamp_mode != 'softplus' (the tensor-op route raises the reference's assertion, ray_marcher.py:35)"
    if (_dual_decoder_nets(*decoders) if dual else _decoder_nets(*decoders)) is None:
        return f"decoder {' + '.join(type(d).__name__ for d in decoders)} is not " + ('OSGDecoder(64) + OSGDecoder_semantic(32)' if dual else 'an OSG 32-64-33 decoder')
    return None


class Route(NamedTuple):
    kind: str                      # 'fused': one launch | 'fused_autograd': the same forward inside _FusedRenderFn / _FusedPointsFn | 'tensor_ops'
    reason: Optional[str]          # why not fused; None when fused
    expand: bool                   # planes of batch 1 serve B ray sets: True = broadcast them first (only the graph-less fused launch reads the one set in place)


def render_route(entry, policy, on_device, needs_grad, has_backward, plane_shapes, n_rays, options, decoders, who='ImportanceRenderer'):
    """What one call of ``entry`` ('forward' | 'run_model' | 'dual_forward' | 'dual_run_model') runs on, from facts only.  ``needs_grad``: the call is part of
    an autograd graph; ``has_backward``: this entry point can give that graph a fused backward (``fused_training``; never for a gradient w.r.t. point
    coordinates, never for two plane sets).  Raises the batch-mismatch ``ValueError`` of ``shared_planes`` for the ray entry points (point queries take the
    planes' batch as it comes)."""
    dual, rays = entry.startswith('dual'), entry.endswith('forward')
    shared = False
    if rays and (dual or len(plane_shapes[0]) == 5):
        shared = any([shared_planes(s[0], n_rays, who, allowed=not dual) for s in plane_shapes])
    reason = fallback_reason(policy, on_device, options, decoders, graph=needs_grad and not has_backward, plane_shapes=plane_shapes)
    if reason is None and rays:
        sc, sf = int(options['depth_resolution']), int(options['depth_resolution_importance'])
        if not (4 <= sc <= 64 and 1 <= sf <= 64):
            reason = 'sample counts outside the fused kernel envelope (4..64 coarse, 1..64 fine)'
    kind = 'tensor_ops' if reason is not None else ('fused_autograd' if needs_grad else 'fused')
    return Route(kind, reason, shared and kind != 'fused')


def _needs_grad(tensors, decoders):
    return torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or any(p.requires_grad for d in decoders for p in d.parameters()))


# ---- the operands of every launch -------------------------------------------------------------------------------------------------
def render_desc(n_img, rays_per_img, plane_h, plane_w, strides, n_nets, semantic_sigmoid, mode, options, numeric_limits=False, raster=0):
    """p3d_render_desc from shapes, plane strides, decoder form, MLP mode and options.  ``numeric_limits``: the rays run from options['ray_start'] to
    ['ray_end'] (else per-ray limits travel as tensors, or — point queries — there are no rays); ``raster`` is a pure scheduling hint, plus
    P3D_RENDER_SHARED_PLANES."""
    start, end = (options['ray_start'], options['ray_end']) if numeric_limits else (0.0, 0.0)
    return _RenderDesc(n_img, rays_per_img, plane_h, plane_w, n_nets, int(semantic_sigmoid), int(options.get('depth_resolution', 0)),
                       int(options.get('depth_resolution_importance', 0)), int(bool(options.get('disparity_space_sampling', False))),
                       int(bool(options.get('white_back', False))), float(start), float(end), float(options['box_warp']), *strides, int(raster), int(mode))


def _plane_set_cl(planes):
    """[N,3,32,H,W] planes as the kernels read them: (tensor, (image, plane, pixel) strides in floats).  A channels-last [N,96,H,W]
    backbone output viewed as [N,3,32,H,W] is read in place; anything else goes through one re-layout pass to [N][3][H][W][32]."""
    n, k, c, h, w = planes.shape
    assert k == 3 and c == 32
    st = planes.stride()
    if planes.dtype == torch.float32 and st[2] == 1 and st[1] == 32 and st[4] >= 96 and st[3] == w * st[4] and st[0] == h * st[3] and st[4] % 4 == 0 \
            and planes.data_ptr() % 16 == 0:
        return planes.detach(), (st[0], st[1], st[4])
    src = _f32c(planes)
    out = torch.empty([n, 3, h, w, 32], dtype=torch.float32, device=planes.device)
    _lib.check(_lib.lib().p3d_planes_to_channels_last(_lib.ptr(src), _lib.ptr(out), n, h, w, _lib.stream_of(src)), 'planes_to_channels_last')
    return out, (0, 0, 0)


class _FusedContext:
    """Device-side operands shared by the fused entry points: texel-major planes + packed decoder + descriptor.  ``decoder_info``: ``_decoder_nets``'
    result, or — with ``planes_semantic`` — ``_dual_decoder_nets``' for the two-plane-set kernels."""

    def __init__(self, planes, decoder_info, bf16x3=0, planes_semantic=None):
        nets, lr_mul, self.sem_sigmoid = decoder_info
        dual = planes_semantic is not None
        self.bf16x3 = 0 if dual else int(bf16x3)                # p3d_render_desc.mlp_bf16x3: 0 exact, 1 bf16x3, 2 layer 1 as bf16x6
        self.n, _, _, self.h, self.w = planes.shape
        self.n_nets = len(nets)
        self.planes_cl, self.strides = _plane_set_cl(planes)
        if dual:
            self.planes_semantic_cl, st = _plane_set_cl(planes_semantic)
            if st != self.strides:                               # one descriptor describes both sets: bring the odd one to the default layout
                if self.strides != (0, 0, 0):
                    self.planes_cl, self.strides = _plane_set_cl(planes.contiguous())
                if st != (0, 0, 0):
                    self.planes_semantic_cl, _ = _plane_set_cl(planes_semantic.contiguous())
        # the FullyConnectedLayer parameters in the kernels' LDS image, on the current stream
        lib = _lib.lib()
        self._keep = [_f32c(t) for fc1, fc2 in nets for t in (fc1.weight, fc1.bias, fc2.weight, fc2.bias)]
        ptrs = [_lib.ptr(t) for t in self._keep] + [None] * (8 - len(self._keep))
        self.packed = torch.empty([lib.p3d_render_decoder_floats_dual() if dual else lib.p3d_render_decoder_floats()], dtype=torch.float32, device=planes.device)
        if dual:
            code = lib.p3d_pack_decoder_dual(*ptrs, lr_mul, _lib.ptr(self.packed), _lib.stream_of(self.packed))
        else:
            pack = (lib.p3d_pack_decoder, lib.p3d_pack_decoder_bf16x3, lib.p3d_pack_decoder_l1x6)[self.bf16x3]
            code = pack(*ptrs, len(nets), lr_mul, _lib.ptr(self.packed), _lib.stream_of(self.packed))
        _lib.check(code, 'pack_decoder_dual' if dual else 'pack_decoder')

    def desc(self, options, rays_per_img=1, numeric_limits=False, raster=0, n_img=None):
        return render_desc(self.n if n_img is None else n_img, rays_per_img, self.h, self.w, self.strides, self.n_nets, self.sem_sigmoid, self.bf16x3, options,
                           numeric_limits, raster)


def _flat_limits(t):
    """Per-ray near / far limits as the kernels read them: flat fp32, or None for numeric limits."""
    return None if t is None else _f32c(t).reshape(-1)


def _ray_outputs(n, m, channels, device):
    """(feat [N,M,C], depth [N,M,1], wsum [N,M,1], the launch-wide depth min / max the kernel clamps with)."""
    return (torch.empty([n, m, channels], device=device, dtype=torch.float32), torch.empty([n, m, 1], device=device, dtype=torch.float32),
            torch.empty([n, m, 1], device=device, dtype=torch.float32), torch.empty([2], device=device, dtype=torch.int32))


def _plane_grad(d_planes, planes):
    """The channels-last gradient as a gradient of ``planes``: a [N,3,32,H,W] view, contiguous if the planes were."""
    g_planes = d_planes.permute(0, 1, 4, 2, 3)
    return g_planes.contiguous() if planes.dim() == 5 and planes.is_contiguous() else g_planes


def _draw_uniforms(n, m, sc, sf, device, tensor_limits):
    """The reference's two draws, in its order: rand_like(depths_coarse) [N,M,Sc,1] (renderer.py:190) then sample_pdf's rand(N*M, Sf) (:237).  With tensor
    limits the reference's rand_like fills a permuted [S,N,M,1] linspace in ITS memory order (:184-186)."""
    if tensor_limits:
        u_c = torch.rand([sc, n, m, 1], device=device, dtype=torch.float32).permute(1, 2, 0, 3)
    else:
        u_c = torch.rand([n, m, sc, 1], device=device, dtype=torch.float32)
    return u_c, torch.rand([n * m, sf], device=device, dtype=torch.float32)


class ImportanceRenderer(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.ray_marcher = MipRayMarcher2()
        self.plane_axes = generate_planes()

    # ------------------------------------------------------------------------------------------------
    def _route(self, entry, plane_sets, decoders, tensors, n_rays, options, has_backward):
        """``render_route`` for this call's tensors, and the plane sets as its route reads them (shared planes outside the graph-less fused launch:
        broadcast, as if they had been repeated)."""
        route = render_route(entry, fused_policy, plane_sets[0].device.type == 'cuda', _needs_grad(plane_sets + tensors, decoders), has_backward,
                             [p.shape for p in plane_sets], n_rays, options, decoders, who=type(self).__name__)
        if route.expand:
            plane_sets = [p.expand(n_rays, -1, -1, -1, -1) for p in plane_sets]
        if route.reason is not None:
            _tensor_op_guard(type(self).__name__, plane_sets[0].device.type == 'cuda', route.reason)
        return route, plane_sets

    def forward(self, planes, decoder, ray_origins, ray_directions, rendering_options):
        self.plane_axes = self.plane_axes.to(ray_origins.device)
        route, (planes,) = self._route('forward', [planes], (decoder,), [ray_origins, ray_directions], ray_origins.shape[0], rendering_options, fused_training)
        if route.kind == 'tensor_ops':
            return self._forward_tensor_ops(planes, decoder, ray_origins, ray_directions, rendering_options)
        u_c, u_f, t0, t1 = self._fused_draws(ray_origins, ray_directions, rendering_options)
        if route.kind == 'fused_autograd':
            return _FusedRenderFn.apply(self, decoder, rendering_options, u_c, u_f, t0, t1, planes, ray_origins, ray_directions, *decoder.parameters())
        return fused_render(planes, decoder, ray_origins, ray_directions, rendering_options, u_c, u_f, t0, t1)

    # ------------------------------------------------------------------------------------------------
    def _ray_limits(self, ray_origins, ray_directions, opt):
        """('auto' branch, renderer.py:91-97) per-ray near/far from the box, invalid rays patched."""
        t0, t1 = math_utils.get_ray_limits_box(ray_origins, ray_directions, box_side_length=opt['box_warp'])
        ok = t1 > t0
        if torch.any(ok).item():
            t0[~ok] = t0[ok].min()
            t1[~ok] = t0[ok].max()
        return t0, t1

    def _fused_draws(self, ray_origins, ray_directions, opt):
        """What a fused ray launch takes besides planes, decoder and rays: (u_coarse, u_fine, t_start, t_end).  The limits come first, as in the reference:
        ``_ray_limits`` synchronises, and the draws keep their place after it."""
        n, m, _ = ray_origins.shape
        t0 = t1 = None
        if opt['ray_start'] == opt['ray_end'] == 'auto':
            t0, t1 = self._ray_limits(ray_origins, ray_directions, opt)
        u_c, u_f = _draw_uniforms(n, m, int(opt['depth_resolution']), int(opt['depth_resolution_importance']), ray_origins.device, t0 is not None)
        return u_c, u_f, t0, t1

    # ------------------------------------------------------------------------------------------------
    def _forward_tensor_ops(self, planes, decoder, ray_origins, ray_directions, opt, point_fn=None):
        """The differentiable tensor-op restatement of forward().  ``point_fn(points, directions) -> {'rgb', 'sigma'}`` replaces the
        plane lookup + decoder (ImportanceSemanticRenderer)."""
        if opt['ray_start'] == opt['ray_end'] == 'auto':
            t0, t1 = self._ray_limits(ray_origins, ray_directions, opt)
            z_c = self.sample_stratified(ray_origins, t0, t1, opt['depth_resolution'], opt['disparity_space_sampling'])
        else:
            z_c = self.sample_stratified(ray_origins, opt['ray_start'], opt['ray_end'], opt['depth_resolution'], opt['disparity_space_sampling'])
        n, m, sc, _ = z_c.shape

        def decode(z):
            s = z.shape[2]
            pts = (ray_origins.unsqueeze(-2) + z * ray_directions.unsqueeze(-2)).reshape(n, -1, 3)
            dirs = ray_directions.unsqueeze(-2).expand(-1, -1, s, -1).reshape(n, -1, 3)
            if point_fn is not None:
                out = point_fn(pts, dirs)
            elif torch.is_grad_enabled():                    # this method IS the tensor-op formulation: under autograd its point queries are tensor ops too
                out = self._points_tensor_ops(planes, decoder, pts, dirs, opt)      # (the replay backward and the tests' reference runs rely on that)
            else:
                out = self.run_model(planes, decoder, pts, dirs, opt)
            return out['rgb'].reshape(n, m, s, -1), out['sigma'].reshape(n, m, s, 1)

        c_c, s_c = decode(z_c)
        sf = opt['depth_resolution_importance']
        if sf > 0:
            _, _, w = self.ray_marcher(c_c, s_c, z_c, opt)
            z_f = self.sample_importance(z_c, w, sf)
            c_f, s_f = decode(z_f)
            z_all, c_all, s_all = self.unify_samples(z_c, c_c, s_c, z_f, c_f, s_f)
            rgb, depth, w = self.ray_marcher(c_all, s_all, z_all, opt)
        else:
            rgb, depth, w = self.ray_marcher(c_c, s_c, z_c, opt)
        return rgb, depth, w.sum(2)

    def run_model(self, planes, decoder, sample_coordinates, sample_directions, options):
        """Sample the planes at 3-D points and decode: {'rgb': [N,P,C], 'sigma': [N,P,1]} (renderer.py:142-148)."""
        self.plane_axes = self.plane_axes.to(sample_coordinates.device)
        # a graph that needs gradients (the density regularisation, loss.py:681-706) takes the fused forward + p3d_sample_points_backward;
        # only a gradient w.r.t. the coordinates themselves has no fused form
        route, (planes,) = self._route('run_model', [planes], (decoder,), [sample_coordinates], sample_coordinates.shape[0], options,
                                       fused_training and not sample_coordinates.requires_grad)
        if route.kind == 'tensor_ops':
            return self._points_tensor_ops(planes, decoder, sample_coordinates, sample_directions, options)
        if route.kind == 'fused_autograd':
            rgb, sigma = _FusedPointsFn.apply(decoder, options, sample_coordinates, planes, *decoder.parameters())
        else:
            rgb, sigma = fused_sample_points(planes, decoder, sample_coordinates, options)
        return {'rgb': rgb, 'sigma': sigma}

    def _points_tensor_ops(self, planes, decoder, sample_coordinates, sample_directions, options):
        """run_model as the reference writes it (renderer.py:142-148): grid_sample + decoder, differentiable in everything."""
        self.plane_axes = self.plane_axes.to(sample_coordinates.device)
        feats = sample_from_planes(self.plane_axes, planes, sample_coordinates, padding_mode='zeros', box_warp=options['box_warp'])
        out = decoder(feats, sample_directions)
        if options.get('density_noise', 0) > 0:
            out['sigma'] += torch.randn_like(out['sigma']) * options['density_noise']
        return out

    # ------------------------------------------------------------------------------------------------
    @staticmethod
    def _sorted_gather(depths, colors, densities):
        _, order = torch.sort(depths, dim=-2)
        take = lambda t: torch.gather(t, -2, order.expand(-1, -1, -1, t.shape[-1]))
        return take(depths), take(colors), take(densities)

    def sort_samples(self, all_depths, all_colors, all_densities):
        return self._sorted_gather(all_depths, all_colors, all_densities)

    def unify_samples(self, depths1, colors1, densities1, depths2, colors2, densities2):
        """Concatenate both sample sets along the ray and order them by depth (renderer.py:157-167)."""
        return self._sorted_gather(torch.cat([depths1, depths2], dim=-2), torch.cat([colors1, colors2], dim=-2),
                                   torch.cat([densities1, densities2], dim=-2))

    def sample_stratified(self, ray_origins, ray_start, ray_end, depth_resolution, disparity_space_sampling=False):
        """Jittered, evenly spaced depths [N,M,S,1]; one uniform per sample (renderer.py:169-192)."""
        n, m, _ = ray_origins.shape
        dev, s = ray_origins.device, depth_resolution
        if disparity_space_sampling:
            t = torch.linspace(0, 1, s, device=dev).reshape(1, 1, s, 1).repeat(n, m, 1, 1)
            t += torch.rand_like(t) * (1 / (s - 1))
            return 1. / (1. / ray_start * (1. - t) + 1. / ray_end * t)
        if isinstance(ray_start, torch.Tensor):
            z = math_utils.linspace(ray_start, ray_end, s).permute(1, 2, 0, 3)
            z += torch.rand_like(z) * ((ray_end - ray_start) / (s - 1))[..., None]
            return z
        z = torch.linspace(ray_start, ray_end, s, device=dev).reshape(1, 1, s, 1).repeat(n, m, 1, 1)
        z += torch.rand_like(z) * ((ray_end - ray_start) / (s - 1))
        return z

    def sample_importance(self, z_vals, weights, N_importance):
        """Importance depths from the coarse weights [N,M,S_f,1], detached (renderer.py:194-212)."""
        with torch.no_grad():
            n, m, s, _ = z_vals.shape
            z = z_vals.reshape(n * m, s)
            w = weights.reshape(n * m, -1)
            w = torch.nn.functional.max_pool1d(w.unsqueeze(1).float(), 2, 1, padding=1)
            w = torch.nn.functional.avg_pool1d(w, 2, 1).squeeze(1) + 0.01
            mids = 0.5 * (z[:, :-1] + z[:, 1:])
            return self.sample_pdf(mids, w[:, 1:-1], N_importance).detach().reshape(n, m, N_importance, 1)

    def sample_pdf(self, bins, weights, N_importance, det=False, eps=1e-5):
        """Inverse-CDF sampling of ``N_importance`` depths per ray (renderer.py:214-253)."""
        rays, nb = weights.shape
        w = weights + eps
        cdf = torch.cumsum(w / w.sum(-1, keepdim=True), -1)
        cdf = torch.cat([torch.zeros_like(cdf[:, :1]), cdf], -1)
        if det:
            u = torch.linspace(0, 1, N_importance, device=bins.device).expand(rays, N_importance)
        else:
            u = torch.rand(rays, N_importance, device=bins.device)
        u = u.contiguous()
        idx = torch.searchsorted(cdf, u, right=True)
        lo, hi = (idx - 1).clamp_min(0), idx.clamp_max(nb)
        c0, c1 = cdf.gather(1, lo), cdf.gather(1, hi)
        b0, b1 = bins.gather(1, lo), bins.gather(1, hi)
        span = c1 - c0
        span = torch.where(span < eps, torch.ones_like(span), span)
        return b0 + (u - c0) / span * (b1 - b0)


class ImportanceSemanticRenderer(ImportanceRenderer):
    """Renderer of the two-backbone generator (reference: renderer.py:256-438): a texture plane set and a semantic plane set; the label
    decoder reads the semantic features and provides density + labels, the colour decoder reads cat(texture, semantic).  Sampling
    and compositing are ImportanceRenderer's, over the feature vector cat(colour, label).

    Device tensors without an autograd graph run the DUAL variant of the fused kernel (``p3d_render_forward_dual`` /
    ``p3d_sample_points_dual``, csrc/render_device.h): both plane sets are gathered per sample, the colour net's first layer takes its
    64 inputs as two 32-wide MFMA blocks.  Graphs that need gradients (train.py no longer selects this generator, :375) and CPU tensors
    take the tensor-op formulation."""

    def forward(self, planes_texture, planes_semantic, decoder_texture, decoder_semantic, ray_origins, ray_directions, rendering_options):
        self.plane_axes = self.plane_axes.to(ray_origins.device)
        route, _ = self._route('dual_forward', [planes_texture, planes_semantic], (decoder_texture, decoder_semantic), [ray_origins, ray_directions],
                               ray_origins.shape[0], rendering_options, False)
        if route.kind == 'fused':
            return fused_render_dual(planes_texture, planes_semantic, decoder_texture, decoder_semantic, ray_origins, ray_directions, rendering_options,
                                     *self._fused_draws(ray_origins, ray_directions, rendering_options))

        def point_fn(pts, dirs):
            out = self._run_model_tensor_ops(planes_texture, planes_semantic, decoder_texture, decoder_semantic, pts, dirs, rendering_options)
            return {'rgb': torch.cat([out['rgb'], out['semantic']], dim=-1), 'sigma': out['sigma']}
        return self._forward_tensor_ops(None, None, ray_origins, ray_directions, rendering_options, point_fn=point_fn)

    def run_model(self, planes_texture, planes_semantic, decoder_texture, decoder_semantic, sample_coordinates, sample_directions, options):
        """-> {'rgb': [N,P,32], 'sigma': [N,P,1], 'semantic': [N,P,32]}  (renderer.py:324-333)."""
        self.plane_axes = self.plane_axes.to(sample_coordinates.device)
        route, _ = self._route('dual_run_model', [planes_texture, planes_semantic], (decoder_texture, decoder_semantic), [sample_coordinates],
                               sample_coordinates.shape[0], options, False)
        if route.kind != 'fused':
            return self._run_model_tensor_ops(planes_texture, planes_semantic, decoder_texture, decoder_semantic, sample_coordinates, sample_directions, options)
        both, sigma = fused_sample_points_dual(planes_texture, planes_semantic, decoder_texture, decoder_semantic, sample_coordinates, options)
        return {'sigma': sigma, 'rgb': both[..., :32], 'semantic': both[..., 32:]}

    def _run_model_tensor_ops(self, planes_texture, planes_semantic, decoder_texture, decoder_semantic, sample_coordinates, sample_directions, options):
        tex = sample_from_planes(self.plane_axes, planes_texture, sample_coordinates, padding_mode='zeros', box_warp=options['box_warp'])
        sem = sample_from_planes(self.plane_axes, planes_semantic, sample_coordinates, padding_mode='zeros', box_warp=options['box_warp'])
        label = decoder_semantic(sem, sample_directions)
        colour = decoder_texture(torch.cat([tex, sem], dim=-1), sample_directions)
        out = {'sigma': label['sigma'], 'rgb': colour['rgb'], 'semantic': label['rgb']}
        if options.get('density_noise', 0) > 0:
            out['sigma'] = out['sigma'] + torch.randn_like(out['sigma']) * options['density_noise']
        return out


def importance_sample_native(z_coarse, w_coarse, u_fine, sort=False):
    """p3d_importance_sample on device tensors: z [R,Sc], w [R,Sc-1], u [R,Sf] -> z_fine [R,Sf]."""
    z, w, u = _f32c(z_coarse), _f32c(w_coarse), _f32c(u_fine)
    out = torch.empty_like(u)
    code = _lib.lib().p3d_importance_sample(_lib.ptr(z), _lib.ptr(w), _lib.ptr(u), _lib.ptr(out), z.shape[0], z.shape[1], u.shape[1], int(sort), _lib.stream_of(z))
    _lib.check(code, 'importance_sample')
    return out


def importance_sample_index_native(z_coarse, w_coarse, u_fine):
    """p3d_importance_sample_index: (sorted z_fine [R,Sf], bin index per draw [R,Sf] int32, merge pattern [R,Sc+Sf] bool: True where the k-th sample of
    the merged ray is an importance sample) — the integer side of sample_pdf / unify_samples, for the parity tests."""
    z, w, u = _f32c(z_coarse), _f32c(w_coarse), _f32c(u_fine)
    out = torch.empty_like(u)
    bins = torch.empty(u.shape, dtype=torch.int32, device=u.device)
    words = torch.empty([u.shape[0], 4], dtype=torch.int32, device=u.device)
    code = _lib.lib().p3d_importance_sample_index(_lib.ptr(z), _lib.ptr(w), _lib.ptr(u), _lib.ptr(out), _lib.ptr(bins), _lib.ptr(words), z.shape[0], z.shape[1], u.shape[1], 1,
                                                  _lib.stream_of(z))
    _lib.check(code, 'importance_sample_index')
    k = torch.arange(z.shape[1] + u.shape[1], device=u.device)
    merged = ((words[:, (k >> 5)] >> (k & 31)) & 1).bool()
    return out, bins, merged


class _replay_draws:
    """Make torch.rand_like / torch.rand hand back given tensors, in order (the renderer's two uniform draws): logical [N,M,Sc,1] / [N*M,Sf] draws, whichever
    way a route asks for them — the tensor-limits branch of the fused route draws [Sc,N,M,1] and permutes (``_draw_uniforms``) and gets the permuted view."""

    def __init__(self, *draws):
        self.draws = list(draws)

    def __enter__(self):
        self._rl, self._r = torch.rand_like, torch.rand
        it = iter(self.draws)

        def rand(*size, **kw):
            size = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (list, tuple, torch.Size)) else tuple(size)
            u = next(it)
            if u.ndim == 4 and size == (u.shape[2], u.shape[0], u.shape[1], 1) and size != tuple(u.shape):
                return u.permute(2, 0, 1, 3)
            return u.reshape(size)
        torch.rand_like = lambda t, *a, **k: next(it).to(t.device).reshape(t.shape)
        torch.rand = rand
        return self

    def __exit__(self, *exc):
        torch.rand_like, torch.rand = self._rl, self._r


backward_calls = {'fused': 0, 'replay': 0, 'points': 0}      # which backward _FusedRenderFn took (tests: the training step must take 'fused'); 'points': _FusedPointsFn


class _FusedRenderFn(torch.autograd.Function):
    """Training-mode rendering: the FORWARD is the fused kernel and keeps nothing per-sample (the reference holds ~1.2 GB of
    sampled features per image for autograd); the BACKWARD recomputes on the device — ``p3d_render_backward``: the forward
    sweep again with a tape, then a point-wise MFMA backward (csrc/render_bwd.hip) — and returns gradients for the planes and
    the decoder parameters.  If a gradient w.r.t. the rays or the depth output is requested (no training loss does), or with
    ``fused_backward = False``, it replays the differentiable tensor-op renderer on the same draws under autograd instead."""

    @staticmethod
    def forward(ctx, renderer, decoder, opt, u_c, u_f, t0, t1, planes, ray_o, ray_d, *params):
        out = fused_render(planes, decoder, ray_o, ray_d, opt, u_c, u_f, t0, t1, exact_fp32=True)
        if out is None:
            raise RuntimeError('fused training render: sample counts outside the kernel envelope')
        ctx.renderer, ctx.decoder, ctx.opt = renderer, decoder, opt
        ctx.limits = (t0, t1)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(u_c, u_f, planes, ray_o, ray_d)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable          # the device kernels are not differentiable: a double backward must raise, not return zeros
    def backward(ctx, g_feat, g_depth, g_wsum):
        u_c, u_f, planes, ray_o, ray_d = ctx.saved_tensors
        params = [p for p in ctx.decoder.parameters()]
        rays_need_grad = ctx.needs_input_grad[8] or ctx.needs_input_grad[9]
        if fused_backward and g_depth is None and not rays_need_grad and g_feat is not None:
            backward_calls['fused'] += 1
            g_planes, g_params = fused_render_backward(planes, ctx.decoder, ray_o, ray_d, ctx.opt, u_c, u_f, ctx.limits[0], ctx.limits[1], g_feat, g_wsum)
            return (None,) * 7 + (g_planes if ctx.needs_input_grad[7] else None, None, None) + tuple(g_params)
        # depth gradients / ray gradients: the differentiable tensor-op renderer, replayed on the same draws
        backward_calls['replay'] += 1
        n, m = ray_o.shape[0], ray_o.shape[1]
        dev = planes.device
        nch = 32 * len(_decoder_nets(ctx.decoder)[0])
        g_feat = torch.zeros([n, m, nch], device=dev) if g_feat is None else g_feat
        g_depth = torch.zeros([n, m, 1], device=dev) if g_depth is None else g_depth
        g_wsum = torch.zeros([n, m, 1], device=dev) if g_wsum is None else g_wsum
        with torch.enable_grad():
            pl = planes.detach().requires_grad_(ctx.needs_input_grad[7])
            ro = ray_o.detach().requires_grad_(ctx.needs_input_grad[8])
            rd = ray_d.detach().requires_grad_(ctx.needs_input_grad[9])
            with _replay_draws(u_c, u_f):
                feat, depth, wsum = ctx.renderer._forward_tensor_ops(pl, ctx.decoder, ro, rd, ctx.opt)
            wanted = [t for t in [pl, ro, rd] + params if t.requires_grad]
            grads = torch.autograd.grad([feat, depth, wsum], wanted, [g_feat, g_depth, g_wsum], allow_unused=True)
        it = iter(grads)
        res = [next(it) if t.requires_grad else None for t in [pl, ro, rd] + params]
        return (None,) * 7 + tuple(res)


def fused_sample_points(planes, decoder, coordinates, opt):
    """One launch of p3d_sample_points: (rgb [N,P,32*n_nets], sigma [N,P,1]) at coordinates [N,P,3] (exact fp32 MFMA decoder)."""
    n, p, _ = coordinates.shape
    ctx = _FusedContext(planes, _decoder_nets(decoder))
    xyz = _f32c(coordinates)
    rgb = torch.empty([n, p, 32 * ctx.n_nets], device=planes.device, dtype=torch.float32)
    sigma = torch.empty([n, p, 1], device=planes.device, dtype=torch.float32)
    d = ctx.desc(opt)
    code = _lib.lib().p3d_sample_points(_lib.ptr(ctx.planes_cl), _lib.ptr(ctx.packed), _lib.ptr(xyz), ctypes.byref(d), p,
                                        _lib.ptr(rgb), _lib.ptr(sigma), _lib.stream_of(rgb))
    _lib.check(code, 'sample_points')
    return rgb, sigma


def fused_sample_lattice(planes, decoder, xs, ys, zs, opt):
    """One launch of p3d_sample_lattice: sigma [N, len(xs), len(ys), len(zs)], the density at every lattice point (xs[i], ys[j], zs[k])
    — what ``fused_sample_points(...)[1]`` gives at those points, without the colour outputs (csrc/shape.hip)."""
    ctx = _FusedContext(planes, _decoder_nets(decoder))
    axes = [_f32c(t).to(planes.device) for t in (xs, ys, zs)]
    sigma = torch.empty([ctx.n] + [len(t) for t in axes], device=planes.device, dtype=torch.float32)
    d = ctx.desc(opt)
    code = _lib.lib().p3d_sample_lattice(_lib.ptr(ctx.planes_cl), _lib.ptr(ctx.packed), ctypes.byref(d), *[_lib.ptr(t) for t in axes],
                                         *[len(t) for t in axes], _lib.ptr(sigma), _lib.stream_of(sigma))
    _lib.check(code, 'sample_lattice')
    return sigma


def fused_surface_cast(planes, decoder, ray_o, ray_d, opt, near, far, steps, refine, threshold, eps, half_box=0.0, raster_width=0):
    """One launch of p3d_surface_cast (csrc/surface.hip; the contract is include/p3d_hip.h's): rays [N, M, 3] against planes of batch N, or of batch 1
    for every ray set (many cameras of one latent) -> (hit uint8 [N, M], depth float32 [N, M], position, grad float32 [N, M, 3]).  Every density the
    cast compares or differences is ``fused_sample_points(...)[1]`` at the same point.  ``half_box <= 0``: no box clip; ``raster_width`` = R when
    the M rays are an R x R image with R % 8 == 0 (scheduling only)."""
    n, m, _ = ray_o.shape
    shared = shared_planes(planes.shape[0], n, 'fused_surface_cast')
    ctx = _FusedContext(planes, _decoder_nets(decoder))
    o, d = _f32c(ray_o), _f32c(ray_d)
    dev = planes.device
    hit = torch.empty([n, m], dtype=torch.uint8, device=dev)
    depth = torch.empty([n, m], dtype=torch.float32, device=dev)
    position, grad = torch.empty([n, m, 3], dtype=torch.float32, device=dev), torch.empty([n, m, 3], dtype=torch.float32, device=dev)
    desc = ctx.desc(opt, rays_per_img=m, raster=_lib.P3D_RENDER_SHARED_PLANES if shared else 0, n_img=n)             # the N ray sets all read the one plane set
    dt = (float(far) - float(near)) / (int(steps) - 1) if int(steps) > 1 else 0.0
    code = _lib.lib().p3d_surface_cast(_lib.ptr(ctx.planes_cl), _lib.ptr(ctx.packed), ctypes.byref(desc), _lib.ptr(o), _lib.ptr(d), float(near), dt,
                                       int(steps), int(refine), float(threshold), float(eps), float(half_box), int(raster_width),
                                       _lib.ptr(hit), _lib.ptr(depth), _lib.ptr(position), _lib.ptr(grad), _lib.stream_of(hit))
    _lib.check(code, 'surface_cast')
    return hit, depth, position, grad


def fused_surface_occlusion(planes, decoder, origin, facing, active, directions, opt, reach, steps, threshold, half_box=0.0, raster_width=0):
    """One launch of p3d_surface_occlusion (csrc/surface.hip; the contract is include/p3d_hip.h's): points ``origin`` [N, M, 3] with the directions
    ``facing`` [N, M, 3] their surface faces and the flags ``active`` uint8 [N, M], rays of ``steps`` samples up to ``reach`` along each of
    ``directions`` [N, K, 3], against planes of batch N or of batch 1 for every point set -> (open, total) uint8 [N, M]: per point the directions it
    uses (facing . d > 0) and those of them no sample of which is denser than ``threshold``.  ``half_box`` and ``raster_width`` as for
    ``fused_surface_cast``."""
    n, m, _ = origin.shape
    shared = shared_planes(planes.shape[0], n, 'fused_surface_occlusion')
    dev = planes.device
    o, f, dirs = _f32c(origin), _f32c(facing), _f32c(directions).to(dev)
    act = active.detach().to(device=dev, dtype=torch.uint8).contiguous()
    if tuple(f.shape) != (n, m, 3) or tuple(act.shape) != (n, m) or dirs.ndim != 3 or dirs.shape[0] != n or dirs.shape[2] != 3:
        raise ValueError(f'fused_surface_occlusion: origin {tuple(o.shape)} needs facing [{n}, {m}, 3], active [{n}, {m}] and directions [{n}, K, 3] '
                         f'(got {tuple(f.shape)}, {tuple(act.shape)}, {tuple(dirs.shape)})')
    # the entry point's own limits, checked here as well: preparing its operands (the planes' re-layout, the decoder stream) already launches
    k, steps, raster_width = int(dirs.shape[1]), int(steps), int(raster_width)
    if not (1 <= k <= 255 and 1 <= steps <= 4096):
        raise RuntimeError(f'fused_surface_occlusion: needs 1 <= directions <= 255 and 1 <= steps <= 4096 (got {k}, {steps})')
    if raster_width < 0 or (raster_width > 0 and (raster_width % 8 != 0 or raster_width * raster_width != m)):
        raise RuntimeError(f'fused_surface_occlusion: raster_width {raster_width} must be 0, or a multiple of 8 whose square is the number of points ({m})')
    ctx = _FusedContext(planes, _decoder_nets(decoder))
    open_, total = torch.empty([n, m], dtype=torch.uint8, device=dev), torch.empty([n, m], dtype=torch.uint8, device=dev)
    desc = ctx.desc(opt, rays_per_img=m, raster=_lib.P3D_RENDER_SHARED_PLANES if shared else 0, n_img=n)             # as the cast
    code = _lib.lib().p3d_surface_occlusion(_lib.ptr(ctx.planes_cl), _lib.ptr(ctx.packed), ctypes.byref(desc), _lib.ptr(o), _lib.ptr(f), _lib.ptr(act),
                                            _lib.ptr(dirs), k, float(reach) / steps, steps, float(threshold), float(half_box), raster_width,
                                            _lib.ptr(open_), _lib.ptr(total), _lib.stream_of(open_))
    _lib.check(code, 'surface_occlusion')
    return open_, total


def _decoder_param_grads(decoder, nets, d_dec):
    """Effective-weight gradient record of the device kernels -> gradients of the raw FullyConnectedLayer parameters, in ``decoder.parameters()`` order."""
    stride = _lib.lib().p3d_render_grad_decoder_floats() // 2
    by_param = {}
    for i, (fc1, fc2) in enumerate(nets):
        g = d_dec[i * stride:(i + 1) * stride]
        by_param[id(fc1.weight)] = g[0:2048].reshape(64, 32) * fc1.weight_gain
        by_param[id(fc1.bias)] = g[2048:2112] * fc1.bias_gain
        by_param[id(fc2.weight)] = g[2112:4224].reshape(33, 64) * fc2.weight_gain
        by_param[id(fc2.bias)] = g[4224:4257] * fc2.bias_gain
    return [by_param.get(id(p)) if p.requires_grad else None for p in decoder.parameters()]


def _pack_decoder_bwd(nets, lr_mul, dev):
    lib = _lib.lib()
    packed_bwd = torch.empty([lib.p3d_render_bwd_decoder_floats()], dtype=torch.float32, device=dev)
    w1s = [_f32c(fc1.weight) for fc1, _ in nets] + [None]
    w2s = [_f32c(fc2.weight) for _, fc2 in nets] + [None]
    _lib.check(lib.p3d_pack_decoder_bwd(_lib.ptr(w1s[0]), _lib.ptr(w2s[0]), _lib.ptr(w1s[1]), _lib.ptr(w2s[1]), len(nets), lr_mul, _lib.ptr(packed_bwd),
                                        _lib.stream_of(packed_bwd)), 'pack_decoder_bwd')
    return packed_bwd


def fused_sample_points_backward(planes, decoder, coordinates, opt, g_rgb, g_sigma):
    """dL/dplanes and dL/d(decoder parameters) of ``fused_sample_points`` from dL/drgb [N,P,32*n_nets] and dL/dsigma [N,P,1] (either may be
    None), by one launch of p3d_sample_points_backward (csrc/render_bwd.hip)."""
    info = _decoder_nets(decoder)
    nets, lr_mul, _ = info
    lib = _lib.lib()
    n, p, _ = coordinates.shape
    dev = planes.device
    ctx = _FusedContext(planes, info)
    packed_bwd = _pack_decoder_bwd(nets, lr_mul, dev)
    xyz = _f32c(coordinates)
    gr = None if g_rgb is None else _f32c(g_rgb)
    gs = None if g_sigma is None else _f32c(g_sigma).reshape(-1)
    d_planes = torch.empty([n, 3, ctx.h, ctx.w, 32], dtype=torch.float32, device=dev)
    d_dec = torch.empty([lib.p3d_render_grad_decoder_floats()], dtype=torch.float32, device=dev)
    d = ctx.desc(opt)
    code = lib.p3d_sample_points_backward(_lib.ptr(ctx.planes_cl), _lib.ptr(ctx.packed), _lib.ptr(packed_bwd), _lib.ptr(xyz), ctypes.byref(d), p,
                                          _lib.ptr(gr), _lib.ptr(gs), _lib.ptr(d_planes), _lib.ptr(d_dec), _lib.stream_of(d_planes))
    _lib.check(code, 'sample_points_backward')
    return _plane_grad(d_planes, planes), _decoder_param_grads(decoder, nets, d_dec)


class _FusedPointsFn(torch.autograd.Function):
    """Point queries under autograd (G.sample_mixed in the density regularisation, loss.py:681-706): fused forward, nothing per-point
    kept; the backward recomputes gather + decoder on the device (``p3d_sample_points_backward``) and returns gradients for the
    planes and the decoder parameters."""

    @staticmethod
    def forward(ctx, decoder, opt, coordinates, planes, *params):
        rgb, sigma = fused_sample_points(planes, decoder, coordinates, opt)
        ctx.decoder, ctx.opt = decoder, opt
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(planes, coordinates)
        return rgb, sigma

    @staticmethod
    @torch.autograd.function.once_differentiable          # the device kernels are not differentiable: a double backward must raise, not return zeros
    def backward(ctx, g_rgb, g_sigma):
        planes, coordinates = ctx.saved_tensors
        backward_calls['points'] += 1
        if g_rgb is None and g_sigma is None:
            return (None,) * (4 + len(list(ctx.decoder.parameters())))
        g_planes, g_params = fused_sample_points_backward(planes, ctx.decoder, coordinates, ctx.opt, g_rgb, g_sigma)
        if g_rgb is None:                                    # only the density carries a gradient (the density regularisation): with two nets the
            nets = _decoder_nets(ctx.decoder)[0]             # colour net is not part of the graph — None for its parameters, as autograd reports it
            if len(nets) == 2:
                skip = {id(p) for fc in nets[0] for p in fc.parameters()}
                g_params = [None if id(p) in skip else g for p, g in zip(ctx.decoder.parameters(), g_params)]
        return (None, None, None, g_planes if ctx.needs_input_grad[3] else None) + tuple(g_params)


def fused_render_backward(planes, decoder, ray_origins, ray_directions, opt, u_coarse, u_fine, t_start, t_end, g_feat, g_wsum=None, debug=False):
    """dL/dplanes (same shape and layout class as ``planes``) and dL/d(decoder parameters) (in ``decoder.parameters()`` order) of the
    fused render, by the two recomputing launches of csrc/render_bwd.hip.  Decoder parameters must require grad to get an entry."""
    info = _decoder_nets(decoder)
    nets, lr_mul, _ = info
    lib = _lib.lib()
    n, m, _ = ray_origins.shape
    sc, sf = int(opt['depth_resolution']), int(opt['depth_resolution_importance'])
    s_all = sc + sf
    dev = planes.device
    ctx = _FusedContext(planes, info)
    packed_bwd = _pack_decoder_bwd(nets, lr_mul, dev)
    t0, t1 = _flat_limits(t_start), _flat_limits(t_end)
    ro, rd, uc, uf = _f32c(ray_origins), _f32c(ray_directions), _f32c(u_coarse), _f32c(u_fine)
    gf = _f32c(g_feat)
    gw = None if g_wsum is None else _f32c(g_wsum).reshape(-1)
    tape_i = torch.empty([n * m, s_all - 1, 4], dtype=torch.float32, device=dev)
    tape_s = torch.empty([n * m, s_all, 4], dtype=torch.float32, device=dev)
    d_planes = torch.empty([n, 3, ctx.h, ctx.w, 32], dtype=torch.float32, device=dev)
    d_dec = torch.empty([lib.p3d_render_grad_decoder_floats()], dtype=torch.float32, device=dev)
    d = ctx.desc(opt, rays_per_img=m, numeric_limits=t0 is None, raster=1)
    code = lib.p3d_render_backward(_lib.ptr(ctx.planes_cl), _lib.ptr(ctx.packed), _lib.ptr(packed_bwd), _lib.ptr(ro), _lib.ptr(rd), _lib.ptr(uc), _lib.ptr(uf),
                                   _lib.ptr(t0), _lib.ptr(t1), ctypes.byref(d), _lib.ptr(gf), _lib.ptr(gw), _lib.ptr(tape_i), _lib.ptr(tape_s),
                                   _lib.ptr(d_planes), _lib.ptr(d_dec), _lib.stream_of(d_planes))
    _lib.check(code, 'render_backward')
    g_planes, g_params = _plane_grad(d_planes, planes), _decoder_param_grads(decoder, nets, d_dec)
    if debug:                                                     # the per-sample tape: z, colour weight, dL/dsigma (tests)
        return g_planes, g_params, tape_s
    return g_planes, g_params


def fused_render(planes, decoder, ray_origins, ray_directions, opt, u_coarse, u_fine, t_start=None, t_end=None, debug=False, exact_fp32=False):
    """One launch of the fused ray-marcher with explicit uniforms (u_coarse [N,M,Sc(,1)], u_fine [N*M,Sf]).
    ``planes`` of batch 1 with N > 1 ray sets is the SHARED-PLANE launch (P3D_RENDER_SHARED_PLANES): all N ray sets read the one plane set — a zero image
    stride — with the schedule and the launch-wide depth clamp of a batch of N, exactly as if the planes had been repeated N times, without the copies.
    Returns (feat [N,M,C], depth [N,M,1], wsum [N,M,1]) and, with debug, the sorted fine depths [N*M,Sf] and the
    coarse weights [N*M,Sc-1] the kernel used; with debug='bins' also the searchsorted index of every draw [N*M,Sf] (int32, draw order).
    None when the library reports the sample counts unsupported."""
    info = _decoder_nets(decoder)
    if info is None:
        raise RuntimeError(f'fused_render: unsupported decoder {type(decoder).__name__}')
    n, m, _ = ray_origins.shape
    shared = shared_planes(planes.shape[0], n, 'fused_render')
    sc, sf = int(opt['depth_resolution']), int(opt['depth_resolution_importance'])
    dev = planes.device
    mode = 1 if (mlp_bf16x3 and not exact_fp32) else (2 if (mlp_l1x6 and modconv.f32_x6) else 0)      # (the training forward stays fp32-accurate: its backward recomputes in fp32)
    ctx = _FusedContext(planes, info, bf16x3=mode)
    t0, t1 = _flat_limits(t_start), _flat_limits(t_end)
    ro, rd, uc, uf = _f32c(ray_origins), _f32c(ray_directions), _f32c(u_coarse), _f32c(u_fine)
    assert uc.numel() == n * m * sc and uf.numel() == n * m * sf
    feat, depth, wsum, mm = _ray_outputs(n, m, 32 * ctx.n_nets, dev)
    dbg_f = torch.empty([n * m, sf], device=dev, dtype=torch.float32) if debug else None
    dbg_w = torch.empty([n * m, sc - 1], device=dev, dtype=torch.float32) if debug else None
    dbg_b = torch.empty([n * m, sf], device=dev, dtype=torch.int32) if debug == 'bins' else None
    # raster 1 is a pure scheduling hint; + P3D_RENDER_SHARED_PLANES: the N ray sets all read the one plane set, each keeping its own R x R raster
    d = ctx.desc(opt, rays_per_img=m, numeric_limits=t0 is None, raster=1 | _lib.P3D_RENDER_SHARED_PLANES if shared else 1, n_img=n)
    with _lib.kernel_timer('render_forward', feat):
        if dbg_b is not None:
            code = _lib.lib().p3d_render_forward_debug(_lib.ptr(ctx.planes_cl), _lib.ptr(ctx.packed), _lib.ptr(ro), _lib.ptr(rd), _lib.ptr(uc), _lib.ptr(uf),
                                                       _lib.ptr(t0), _lib.ptr(t1), ctypes.byref(d), _lib.ptr(feat), _lib.ptr(depth), _lib.ptr(wsum),
                                                       _lib.ptr(mm), _lib.ptr(dbg_f), _lib.ptr(dbg_w), _lib.ptr(dbg_b), _lib.stream_of(feat))
        else:
            code = _lib.lib().p3d_render_forward(_lib.ptr(ctx.planes_cl), _lib.ptr(ctx.packed), _lib.ptr(ro), _lib.ptr(rd), _lib.ptr(uc), _lib.ptr(uf),
                                                 _lib.ptr(t0), _lib.ptr(t1), ctypes.byref(d), _lib.ptr(feat), _lib.ptr(depth), _lib.ptr(wsum),
                                                 _lib.ptr(mm), _lib.ptr(dbg_f), _lib.ptr(dbg_w), _lib.stream_of(feat))
    if code == _lib.P3D_ERR_UNSUPPORTED:
        return None
    _lib.check(code, 'render_forward')
    if dbg_b is not None:
        return feat, depth, wsum, dbg_f, dbg_w, dbg_b
    return (feat, depth, wsum, dbg_f, dbg_w) if debug else (feat, depth, wsum)


def fused_render_dual(planes_texture, planes_semantic, decoder_texture, decoder_semantic, ray_origins, ray_directions, opt, u_coarse, u_fine, t_start=None, t_end=None):
    """``fused_render`` over two plane sets (p3d_render_forward_dual, csrc/render_device.h): both sets are gathered per sample, the colour net's first
    layer takes its 64 inputs as two 32-wide MFMA blocks.  feat [N,M,64] = cat(colour, label).  Inference only; no shared-plane form."""
    n, m, _ = ray_origins.shape
    ctx = _FusedContext(planes_texture, _dual_decoder_nets(decoder_texture, decoder_semantic), planes_semantic=planes_semantic)
    t0, t1 = _flat_limits(t_start), _flat_limits(t_end)
    ro, rd, uc, uf = _f32c(ray_origins), _f32c(ray_directions), _f32c(u_coarse), _f32c(u_fine)
    feat, depth, wsum, mm = _ray_outputs(n, m, 64, ctx.packed.device)
    d = ctx.desc(opt, rays_per_img=m, numeric_limits=t0 is None, raster=1)
    code = _lib.lib().p3d_render_forward_dual(_lib.ptr(ctx.planes_cl), _lib.ptr(ctx.planes_semantic_cl), _lib.ptr(ctx.packed), _lib.ptr(ro), _lib.ptr(rd),
                                              _lib.ptr(uc), _lib.ptr(uf), _lib.ptr(t0), _lib.ptr(t1), ctypes.byref(d), _lib.ptr(feat), _lib.ptr(depth),
                                              _lib.ptr(wsum), _lib.ptr(mm), _lib.stream_of(feat))
    _lib.check(code, 'render_forward_dual')
    return feat, depth, wsum


def fused_sample_points_dual(planes_texture, planes_semantic, decoder_texture, decoder_semantic, coordinates, opt):
    """``fused_sample_points`` over two plane sets (p3d_sample_points_dual): (cat(colour, label) [N,P,64], sigma [N,P,1])."""
    n, p, _ = coordinates.shape
    ctx = _FusedContext(planes_texture, _dual_decoder_nets(decoder_texture, decoder_semantic), planes_semantic=planes_semantic)
    both = torch.empty([n, p, 64], device=ctx.packed.device, dtype=torch.float32)
    sigma = torch.empty([n, p, 1], device=ctx.packed.device, dtype=torch.float32)
    d = ctx.desc(opt, raster=1)                              # (the two-plane-set launches have always set the hint, point queries included)
    code = _lib.lib().p3d_sample_points_dual(_lib.ptr(ctx.planes_cl), _lib.ptr(ctx.planes_semantic_cl), _lib.ptr(ctx.packed), _lib.ptr(_f32c(coordinates)),
                                             ctypes.byref(d), p, _lib.ptr(both), _lib.ptr(sigma), _lib.stream_of(both))
    _lib.check(code, 'sample_points_dual')
    return both, sigma
