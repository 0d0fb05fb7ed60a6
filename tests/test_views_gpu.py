"""pix2pix3d_amd.views on the device: p3d_frame_finish against the numpy restatement of the scripts' finishing (0 differing bytes), the shared-plane
launch of the fused ray-marcher against the repeated-plane launch, render_views end to end at bench size against per-view G.synthesis, and its launch counts."""
import numpy as np
import pytest
import torch

from conftest import rel_err, record_error
from model_cases import build_generator, replay_uniforms
from views_cases import numpy_scale, numpy_label, planted_scale_data, planted_label_data, layouts, to_device_same_layout

pytestmark = pytest.mark.gpu


def _cams(G, n, device='cuda'):
    from pix2pix3d_amd import configs
    rk = G.rendering_kwargs
    return torch.tensor(np.stack([configs.orbit_camera(7 * k + 3, radius=rk['avg_camera_radius'], pivot=rk['avg_camera_pivot']) for k in range(n)]),
                        dtype=torch.float32, device=device)


def _same(a, ref, what):
    a = a.cpu().numpy()
    bad = int((a != ref).sum())
    print(what, 'differing bytes', bad, 'of', ref.size)
    assert a.shape == ref.shape and bad == 0, (what, bad)


# ---- 1. p3d_frame_finish -------------------------------------------------------------------------------------------------------
def test_four_jobs_in_one_launch_at_frame_size(hip_lib):
    """A chunk of B = 4 views at 512^2: image, 6-channel label map (planar, with its index), the same label map channels-last from a device palette, and a
    128^2 depth map — one launch."""
    from pix2pix3d_amd import views, _lib
    img, sem, depth = planted_scale_data(4, 3, 512, 512, seed=1), planted_label_data(4, 6, 512, 512, seed=2), torch.rand(4, 1, 128, 128) * 1.4 + 2.0
    depth[0, 0, 0, :3] = torch.tensor([2.25, 3.3, float('nan')])
    pal = torch.from_numpy(np.random.RandomState(0).randint(0, 256, [6, 3]).astype(np.uint8))
    d_img, d_sem, d_cl = img.cuda(), sem.cuda(), to_device_same_layout(layouts[1](sem))
    assert d_cl.stride(1) == 1
    o_img, o_lab, o_idx = (torch.full(s, 99, dtype=torch.uint8, device='cuda') for s in ([4, 512, 512, 3], [4, 512, 512, 3], [4, 512, 512]))
    o_lab2, o_dep = torch.full([4, 512, 512, 3], 99, dtype=torch.uint8, device='cuda'), torch.full([4, 128, 128], 99, dtype=torch.uint8, device='cuda')
    n0 = _lib.launch_count()
    views.frame_finish([views.FrameJob(d_img, o_img), views.FrameJob(d_sem, o_lab, views.LABEL, palette=pal, dst_index=o_idx),
                        views.FrameJob(d_cl, o_lab2, views.LABEL, palette=pal.cuda()), views.FrameJob(depth.cuda(), o_dep, views.SCALE, 2.25, 3.3)])
    torch.cuda.synchronize()
    assert _lib.launch_count() == n0 + 1
    colour, index = numpy_label(sem.numpy(), pal.numpy())
    _same(o_img, numpy_scale(img.numpy(), -1.0, 1.0), 'image')
    _same(o_lab, colour, 'label planar')
    _same(o_idx, index, 'label index')
    _same(o_lab2, colour, 'label channels-last, device palette')
    _same(o_dep, numpy_scale(depth.numpy(), 2.25, 3.3)[..., 0], 'depth')


@pytest.mark.parametrize('layout', layouts)
@pytest.mark.parametrize('c', [1, 3, 2, 6, 19, 64])
@pytest.mark.parametrize('size', [(3, 509), (8, 512)])
def test_every_path_at_odd_sizes_and_alignments_inside_a_canvas(hip_lib, layout, c, size):
    """Every source path x SCALE / LABEL x four source and destination alignments: the rectangle lands where it should, bytes around it stay untouched."""
    from pix2pix3d_amd import views
    h, w = size
    label = c not in (1, 3)
    pal = torch.from_numpy(np.random.RandomState(c).randint(0, 256, [max(c, 2), 3]).astype(np.uint8))
    for shift in range(4):
        x = layout((planted_label_data if label else planted_scale_data)(2, c, h, w + shift, seed=10 * c + shift))[..., shift:]      # source pointer off by `shift` floats
        ref = numpy_label(x.numpy(), pal.numpy()) if label else (numpy_scale(x.numpy(), -1.0, 1.0),)
        bpp = 1 if c == 1 else 3
        x0, y0 = 5 + shift, 2
        store = torch.full([2 * (h + 5) * (w + 13) * bpp + 8], 171, dtype=torch.uint8, device='cuda')
        canvas = store[shift:shift + 2 * (h + 5) * (w + 13) * bpp].view([2, h + 5, w + 13] + ([3] if bpp == 3 else []))                # destination pointer off by `shift` bytes
        istore = torch.full([2 * (h + 5) * (w + 13) + 8], 171, dtype=torch.uint8, device='cuda')
        icanvas = istore[3 - shift:3 - shift + 2 * (h + 5) * (w + 13)].view(2, h + 5, w + 13)
        xd = to_device_same_layout(x)
        assert xd.stride() == x.stride() and xd.data_ptr() % 16 == (4 * x.storage_offset()) % 16
        if label:
            views.frame_finish([views.FrameJob(xd, canvas, views.LABEL, palette=pal, dst_index=icanvas, x0=x0, y0=y0)])
        else:
            views.frame_finish([views.FrameJob(xd, canvas, x0=x0, y0=y0)])
        torch.cuda.synchronize()
        want = np.full(tuple(canvas.shape), 171, np.uint8)
        want[:, y0:y0 + h, x0:x0 + w] = ref[0] if bpp == 3 else ref[0][..., 0]
        assert np.array_equal(canvas.cpu().numpy(), want), (layout.__name__, c, size, shift, int((canvas.cpu().numpy() != want).sum()))
        assert (store[:shift] == 171).all() and (store[shift + canvas.numel():] == 171).all()
        if label:
            iwant = np.full(tuple(icanvas.shape), 171, np.uint8)
            iwant[:, y0:y0 + h, x0:x0 + w] = ref[1]
            assert np.array_equal(icanvas.cpu().numpy(), iwant), (layout.__name__, c, size, shift, 'index')


def test_argument_errors_come_back_as_codes(hip_lib):
    import ctypes
    from pix2pix3d_amd import views
    job = (views._FrameJobC * 1)()
    assert hip_lib.p3d_frame_finish(ctypes.cast(job, ctypes.c_void_p), 1, None) == -2 and b'null pointer' in hip_lib.p3d_last_error()
    assert hip_lib.p3d_frame_finish(ctypes.cast(job, ctypes.c_void_p), 5, None) == -2
    x, d = torch.zeros(1, 3, 4, 4, device='cuda'), torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device='cuda')
    q = job[0]
    q.src, q.dst, q.src_stride = x.data_ptr(), d.data_ptr(), (ctypes.c_int64 * 4)(*x.stride())
    q.mode, q.n, q.c, q.h, q.w, q.x0, q.y0, q.dst_bpp, q.dst_row_pitch, q.dst_frame_pitch = 0, 1, 3, 4, 4, 1, 0, 3, 12, 48
    assert hip_lib.p3d_frame_finish(ctypes.cast(job, ctypes.c_void_p), 1, None) == -2 and b'row pitch' in hip_lib.p3d_last_error()
    q.x0, q.c = 0, 2
    assert hip_lib.p3d_frame_finish(ctypes.cast(job, ctypes.c_void_p), 1, None) == -2
    q.c, q.mode = 65, 1
    assert hip_lib.p3d_frame_finish(ctypes.cast(job, ctypes.c_void_p), 1, None) == -2 and b'2 .. 64' in hip_lib.p3d_last_error()


# ---- 2. the shared-plane launch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [(4, 128), (3, 24)])
def test_shared_plane_launch_equals_the_repeated_plane_launch(hip_lib, case):
    """ONE p3d_render_forward launch over planes [1, ...] for B cameras against today's launch over the planes repeated B times, same explicit draws: the fold
    changes which block takes which ray, never a ray's arithmetic — feat / depth / wsum are compared as bits."""
    from pix2pix3d_amd import _lib
    from pix2pix3d_amd.training.volumetric_rendering import renderer as rmod
    B, nrr = case
    G = build_generator('seg2cat', 'cuda', depth=(64, 64))
    rk = G.rendering_kwargs
    g = torch.Generator().manual_seed(21)
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=g).cuda()
    c = _cams(G, B)
    m = nrr * nrr
    u_c, u_f = torch.rand(B, m, 64, 1, generator=g).cuda(), torch.rand(B * m, 64, generator=g).cuda()
    with torch.no_grad():
        planes = G.backbone_planes(ws, noise_mode='const')
        planes = planes.view(1, 3, 32, planes.shape[-2], planes.shape[-1])
        o, d = G.ray_sampler(c[:, :16].view(-1, 4, 4), c[:, 16:25].view(-1, 3, 3), nrr)
        _lib.kernel_events['render_forward'] = []
        try:
            shared = rmod.fused_render(planes, G.decoder, o, d, rk, u_c, u_f)
            assert len(_lib.kernel_events['render_forward']) == 1                # one launch for the B views
            repeated = rmod.fused_render(planes.expand(B, -1, -1, -1, -1).contiguous(), G.decoder, o, d, rk, u_c, u_f)
        finally:
            _lib.kernel_events.pop('render_forward', None)
        torch.cuda.synchronize()
        assert tuple(shared[0].shape) == (B, m, 64) and tuple(shared[1].shape) == (B, m, 1)
        for name, a, b in zip(('feat', 'depth', 'wsum'), shared, repeated):
            nbits = int((a.view(torch.int32) != b.view(torch.int32)).sum())
            err = rel_err(a.cpu().numpy(), b.cpu().numpy())
            print(case, name, 'values with different bits', nbits, 'rel err', err)
            record_error(f'views.shared_planes.{B}x{nrr}.{name}', {'different_bits': nbits, 'rel_err': err})
            assert nbits == 0, (name, nbits, err)
        n0 = _lib.launch_count()
        with pytest.raises(ValueError, match=r'batch 2.*batch 3'):
            rmod.fused_render(planes.expand(2, -1, -1, -1, -1), G.decoder, o[:3], d[:3], rk, u_c[:3], u_f[:3 * m])
        with pytest.raises(ValueError, match=r'batch 2.*batch 3'):
            G.renderer(planes.expand(2, -1, -1, -1, -1), G.decoder, o[:3], d[:3], rk)
        assert _lib.launch_count() == n0


# ---- 3. end to end at bench size -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,force_fp32', [('seg2cat', True), ('seg2cat', False), ('edge2car', False)])
def test_render_views_equals_per_view_synthesis_at_bench_size(hip_lib, name, force_fp32):
    """render_views (one backbone pass, shared-plane chunks of 4, frozen draws) against G.synthesis per view on the same replayed draws — the route every call took
    before shared planes existed — within the bounds tests/test_model_full.py applies to this arithmetic (1e-4; 3e-3 with fp16 heads; edge2car + fp16 heads
    5e-3 raw / 8e-3); and the uint8 frames are exactly the numpy finishing of the float tensors they were made from.  Fixed ray limits + frozen draws give every
    view the same sample-depth range, so the launch-wide depth clamp equals the per-view one and image_depth is part of the comparison."""
    from pix2pix3d_amd import views
    G = build_generator(name, 'cuda', depth=(64, 64))
    rk = G.rendering_kwargs
    nrr = 128 if name == 'seg2cat' else 64
    g = torch.Generator().manual_seed(31)
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=g).cuda()
    F = 6
    cams = _cams(G, F)
    u = (torch.rand(1, nrr * nrr, 64, 1, generator=g), torch.rand(nrr * nrr, 64, generator=g))
    found = G._last_planes
    out = views.render_views(G, ws, cams, views_per_step=4, jitter=u, neural_rendering_resolution=nrr, return_float=True, noise_mode='const', force_fp32=force_fp32,
                             depth_range=(rk['ray_start'], rk['ray_end']))
    assert G._last_planes is found
    fl = out['float']
    fp16_raw = name == 'edge2car' and not force_fp32
    tol_raw, tol_sr = (5e-3 if fp16_raw else 1e-4), (1e-4 if force_fp32 else (8e-3 if fp16_raw else 3e-3))
    errs = {}
    for i in range(F):
        with replay_uniforms(u[0], u[1]), torch.no_grad():
            one = G.synthesis(ws, cams[i:i + 1], neural_rendering_resolution=nrr, noise_mode='const', force_fp32=force_fp32)
        for k in ('image_raw', 'semantic_raw', 'image', 'semantic'):
            errs[k] = max(errs.get(k, 0.0), rel_err(fl[k][i:i + 1].float().cpu().numpy(), one[k].float().cpu().numpy()))
        errs['image_depth'] = max(errs.get('image_depth', 0.0), float((fl['image_depth'][i:i + 1] - one['image_depth']).abs().max()))
    print(name, 'fp32' if force_fp32 else 'fp16-sr', errs)
    record_error(f'views.render_views.{name}.' + ('fp32' if force_fp32 else 'fp16-sr'), errs)
    assert errs['image_raw'] < tol_raw and errs['semantic_raw'] < tol_raw and errs['image_depth'] < 1e-4, errs
    assert errs['image'] < tol_sr and errs['semantic'] < tol_sr, errs
    _same(out['image'], numpy_scale(fl['image'].float().cpu().numpy(), -1.0, 1.0), 'image frames')
    _same(out['depth'], numpy_scale(fl['image_depth'].float().cpu().numpy(), rk['ray_start'], rk['ray_end'])[..., 0], 'depth frames')
    if name == 'seg2cat':
        from pix2pix3d_amd import mesh
        colour, index = numpy_label(fl['semantic'].float().cpu().numpy(), mesh.default_palette(6).numpy())
        _same(out['label'], colour, 'label frames')
        _same(out['label_index'], index, 'label index')
    else:
        _same(out['label'], numpy_scale(fl['semantic'].float().cpu().numpy(), -1.0, 1.0)[..., 0], 'grey label frames')


# ---- 4. launch counts --------------------------------------------------------------------------------------------------------------------
def test_a_video_is_one_backbone_pass_and_one_ray_marcher_launch_per_chunk(hip_lib):
    from pix2pix3d_amd import views, _lib
    G = build_generator('seg2cat', 'cuda', depth=(64, 64))
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(41)).cuda()
    cams = views.video_cameras(G, 'seg2cat', 120).cuda()
    passes = []
    h = G.backbone.synthesis.register_forward_hook(lambda *a: passes.append(1))
    _lib.kernel_events['render_forward'], _lib.kernel_events['frame_finish'] = [], []
    try:
        out = views.render_views(G, ws, cams, views_per_step=4, neural_rendering_resolution=128, noise_mode='const')
        torch.cuda.synchronize()
        n_render, n_finish = len(_lib.kernel_events['render_forward']), len(_lib.kernel_events['frame_finish'])
    finally:
        h.remove()
        _lib.kernel_events.pop('render_forward', None)
        _lib.kernel_events.pop('frame_finish', None)
    assert len(passes) == 1 and n_render == 30 and n_finish == 30, (len(passes), n_render, n_finish)
    assert tuple(out['image'].shape) == (120, 512, 512, 3) and tuple(out['label_index'].shape) == (120, 512, 512) and out['image'].is_cuda
    assert int(out['label_index'].max()) < 6 and len({int(out['image'][i].sum()) for i in (0, 30, 60, 90)}) > 1
