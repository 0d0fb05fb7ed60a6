"""pix2pix3d_amd.views without a GPU: the torch formulation of the frame finishing against a numpy restatement of the reference scripts' lines, the
video cameras against labels recorded from the reference's LookAtPoseSampler, shared planes on the tensor-op route, and render_views / generate_video."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from model_cases import build_generator
from views_cases import numpy_scale, numpy_label, planted_scale_data, planted_label_data, layouts


# ---- 1. finishing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', layouts)
def test_finish_frames_image_equals_the_scripts_numpy_lines(layout):
    from pix2pix3d_amd import views
    x = layout(planted_scale_data(2, 3, 37, 53, seed=1))
    out = views.finish_frames({'image': x})
    ref = numpy_scale(x.numpy(), -1.0, 1.0)
    assert out['image'].dtype == torch.uint8 and tuple(out['image'].shape) == (2, 37, 53, 3)
    assert np.array_equal(out['image'].numpy(), ref)
    # the scripts' own two spellings are those bytes (NaN aside, which numpy leaves undefined and this package pins to 0)
    xn = x.numpy()
    ok = ~np.isnan(xn).any(axis=1)
    with np.errstate(invalid='ignore'):
        a = ((xn.transpose(0, 2, 3, 1).clip(-1, 1) + 1) * 127.5).astype(np.uint8)            # generate_video.py:65
        b = ((xn + 1) * 127.5).clip(0, 255).astype(np.uint8).transpose(0, 2, 3, 1)            # generate_video.py:81
    assert np.array_equal(a[ok], ref[ok]) and np.array_equal(b[ok], ref[ok])
    assert (ref[~ok][np.isnan(xn.transpose(0, 2, 3, 1)[~ok])] == 0).all()


def test_every_bucket_edge_lands_in_its_bucket():
    from pix2pix3d_amd import views
    k = np.arange(256, dtype=np.float32)
    edges = (k / np.float32(127.5) - np.float32(1)).astype(np.float32)
    x = torch.from_numpy(np.stack([edges, np.nextafter(edges, np.float32(-2)), np.nextafter(edges, np.float32(2))]).reshape(1, 3, 1, 256))
    out = views.finish_frames({'image': x})['image'].numpy()
    assert np.array_equal(out, numpy_scale(x.numpy(), -1.0, 1.0))
    assert out[0, 0, 0, 0] == 0 and out[0, 0, 255, 0] == 255 and out[0, 0, 255, 2] == 255 and out[0, 0, 0, 1] == 0


@pytest.mark.parametrize('c', [2, 6, 19, 64])
@pytest.mark.parametrize('layout', layouts)
def test_finish_frames_labels_equal_argmax_and_palette_loop(c, layout):
    from pix2pix3d_amd import views, mesh
    sem = layout(planted_label_data(2, c, 19, 31, seed=c))
    img = planted_scale_data(2, 3, 19, 31, seed=2)
    pal = torch.from_numpy(np.random.RandomState(c).randint(0, 256, [c, 3]).astype(np.uint8))
    out = views.finish_frames({'image': img, 'semantic': sem}, palette=pal)
    colour, index = numpy_label(sem.numpy(), pal.numpy())
    assert np.array_equal(out['label_index'].numpy(), index) and np.array_equal(out['label'].numpy(), colour)
    assert out['label'].dtype == out['label_index'].dtype == torch.uint8
    dflt = views.finish_frames({'image': img, 'semantic': sem})
    assert np.array_equal(dflt['label'].numpy(), mesh.default_palette(c).numpy()[index])


def test_one_label_channel_is_a_grey_map_and_depth_is_scaled():
    from pix2pix3d_amd import views
    img, sem = planted_scale_data(1, 3, 8, 9, seed=3), planted_scale_data(1, 1, 8, 9, seed=4)
    depth = torch.rand(1, 1, 4, 5) * 1.5 + 2.0
    out = views.finish_frames({'image': img, 'semantic': sem, 'image_depth': depth}, depth_range=(2.25, 3.3))
    assert tuple(out['label'].shape) == (1, 8, 9) and 'label_index' not in out
    assert np.array_equal(out['label'].numpy(), numpy_scale(sem.numpy(), -1.0, 1.0)[..., 0])      # generate_video.py:82
    assert np.array_equal(out['depth'].numpy(), numpy_scale(depth.numpy(), 2.25, 3.3)[..., 0])


def test_frame_finish_writes_rectangles_of_a_canvas_and_rejects_what_does_not_fit():
    from pix2pix3d_amd import views
    x = planted_scale_data(2, 3, 5, 7, seed=5)
    canvas = torch.full([2, 9, 20, 3], 77, dtype=torch.uint8)
    views.frame_finish([views.FrameJob(x, canvas, x0=11, y0=3)])
    ref = np.full([2, 9, 20, 3], 77, np.uint8)
    ref[:, 3:8, 11:18] = numpy_scale(x.numpy(), -1.0, 1.0)
    assert np.array_equal(canvas.numpy(), ref)
    with pytest.raises(ValueError):
        views.frame_finish([views.FrameJob(x, canvas, x0=14, y0=3)])
    with pytest.raises(ValueError):
        views.frame_finish([views.FrameJob(x.double(), canvas)])
    with pytest.raises(ValueError):
        views.frame_finish([views.FrameJob(planted_label_data(2, 6, 5, 7, seed=1), canvas, views.LABEL)])      # no palette


def test_image_grid():
    from pix2pix3d_amd import views
    f = torch.arange(6 * 2 * 3 * 3, dtype=torch.uint8).reshape(6, 2, 3, 3)
    g = views.image_grid(f, (3, 2))
    assert tuple(g.shape) == (4, 9, 3) and torch.equal(g[2:4, 3:6], f[4]) and torch.equal(views.image_grid(f[..., 0], (3, 2))[0:2, 6:9], f[2, ..., 0])


# ---- 2. cameras --------------------------------------------------------------------------------------------------------------
class _Stub:
    def __init__(self, pivot, radius):
        self.rendering_kwargs = dict(avg_camera_pivot=[float(v) for v in pivot], avg_camera_radius=float(radius))


@pytest.mark.parametrize('cfg', ['seg2cat', 'seg2face', 'edge2cat', 'edge2car'])
def test_video_cameras_equal_the_reference_scripts_labels(cfg):
    from pix2pix3d_amd import views
    g = load_golden('views_cameras')
    cams = views.video_cameras(_Stub(g[cfg + '_pivot'], g[cfg + '_radius']), cfg, 120)
    assert cams.dtype == torch.float32 and tuple(cams.shape) == (120, 25)
    err = float(np.abs(cams.numpy() - g[cfg]).max())
    print(cfg, 'max abs difference', err)
    assert err <= 1e-4                                        # (the bound of tests/test_mesh_host.py for turntable_poses)
    with pytest.raises(ValueError):
        views.video_cameras(_Stub([0, 0, 0], 1.0), 'seg2dog')


# ---- 3. shared planes, tensor-op route ------------------------------------------------------------------------------------------
def _cams(G, n):
    from pix2pix3d_amd import configs
    rk = G.rendering_kwargs
    return torch.tensor(np.stack([configs.orbit_camera(11 * k + 2, radius=rk['avg_camera_radius'], pivot=rk['avg_camera_pivot']) for k in range(n)]), dtype=torch.float32)


def _small(name):
    return build_generator(name, 'cpu', cbase=2048, cmax=32, depth=(6, 6), sr_num_fp16_res=0)


@pytest.mark.parametrize('name', ['seg2cat', 'mask_entangled'])
def test_cached_planes_of_batch_one_serve_b_cameras(name):
    """``G.synthesis(ws, c[B], use_cached_backbone=True)`` on cached batch-1 planes == the same call on the planes repeated B times, exactly."""
    if name == 'mask_entangled':
        from pix2pix3d_amd import configs, dnnlib
        from model_cases import weights
        torch.manual_seed(0)
        G = dnnlib.util.construct_class_by_name(**configs.variant_kwargs('mask_entangled')).eval().requires_grad_(False)
        weights.seed_module(G, seed=1)
    else:
        G = _small(name)
    B = 3
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(5))
    c = _cams(G, B)
    found = G._last_planes
    try:
        with torch.no_grad():
            planes = G.backbone.synthesis(ws, noise_mode='const')                  # what cache_backbone keeps
            assert planes.shape[0] == 1
            outs = []
            for cached, w in ((planes, ws), (planes.expand(B, -1, -1, -1).contiguous(), ws.expand(B, -1, -1).contiguous())):
                G._last_planes = cached
                torch.manual_seed(9)
                outs.append(G.synthesis(w, c, neural_rendering_resolution=16, use_cached_backbone=True, noise_mode='const'))
            shared, repeated = outs
            assert set(shared) == set(repeated) and shared['image'].shape[0] == B
            for k in shared:
                assert torch.equal(shared[k], repeated[k]), k
            assert ('semantic' in shared) == (name == 'seg2cat')
            G._last_planes = planes.expand(2, -1, -1, -1).contiguous()
            with pytest.raises(ValueError, match=r'batch 2.*batch 3'):
                G.synthesis(ws.expand(2, -1, -1), c, neural_rendering_resolution=16, use_cached_backbone=True, noise_mode='const')
    finally:
        G._last_planes = found


def test_renderer_rejects_mismatched_batches_before_any_work():
    from pix2pix3d_amd.training.volumetric_rendering import renderer as rmod
    G = _small('seg2cat')
    planes = torch.zeros(2, 3, 32, 8, 8)
    o, d = torch.zeros(3, 16, 3), torch.ones(3, 16, 3)
    with pytest.raises(ValueError, match=r'batch 2.*batch 3'):
        G.renderer(planes, G.decoder, o, d, G.rendering_kwargs)
    with pytest.raises(ValueError, match=r'batch 2.*batch 3'):
        rmod.fused_render(planes, G.decoder, o, d, G.rendering_kwargs, torch.zeros(3, 16, 6, 1), torch.zeros(48, 6))


# ---- 4. render_views ---------------------------------------------------------------------------------------------------------
def test_render_views_frozen_jitter_does_not_depend_on_views_per_step():
    from pix2pix3d_amd import views
    G = _small('seg2cat')
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(6))
    cams = _cams(G, 5)
    marker = object()
    found, G._last_planes = G._last_planes, marker
    calls = []
    h = G.backbone.synthesis.register_forward_hook(lambda *a: calls.append(1))
    try:
        outs = []
        for step in (1, 2, 3):
            torch.manual_seed(3)
            outs.append(views.render_views(G, ws, cams, views_per_step=step, jitter='frozen', neural_rendering_resolution=16, noise_mode='const', depth_range=(2.25, 3.3)))
            assert G._last_planes is marker
        assert len(calls) == 3                                        # one backbone pass per video
    finally:
        h.remove()
        G._last_planes = found
    a = outs[0]
    res = G.img_resolution
    assert tuple(a['image'].shape) == (5, res, res, 3) and tuple(a['label'].shape) == (5, res, res, 3) and tuple(a['label_index'].shape) == (5, res, res)
    assert tuple(a['depth'].shape) == (5, 16, 16) and all(v.dtype == torch.uint8 for v in a.values())
    for b in outs[1:]:
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert len({bytes(a['image'][i].numpy().tobytes()) for i in range(5)}) == 5      # five different views


def test_render_views_takes_a_latent_per_frame_and_returns_the_floats():
    from pix2pix3d_amd import views
    G = _small('seg2cat')
    ws = torch.randn(3, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(7))
    cams = _cams(G, 3)
    calls = []
    h = G.backbone.synthesis.register_forward_hook(lambda m, a, o: calls.append(o.shape[0]))
    try:
        rnd = views.render_views(G, ws, cams, views_per_step=2, neural_rendering_resolution=16, noise_mode='const')
        assert calls == [2, 1]                                        # the equal-batch route per chunk
        torch.manual_seed(4)
        u = (torch.rand(1, 256, 6, 1), torch.rand(256, 6))
        out = views.render_views(G, ws, cams, views_per_step=2, jitter=u, neural_rendering_resolution=16, noise_mode='const', return_float=True)
    finally:
        h.remove()
    assert tuple(rnd['image'].shape) == tuple(out['image'].shape) and not torch.equal(rnd['image'], out['image'])      # other draws
    fl = out['float']
    assert tuple(fl['image'].shape) == (3, 3, G.img_resolution, G.img_resolution) and fl['image'].dtype == torch.float32
    assert np.array_equal(out['image'].numpy(), numpy_scale(fl['image'].numpy(), -1.0, 1.0))
    with torch.no_grad(), views._frozen_draws(u[0], u[1]):
        one = G.synthesis(ws[2:3], cams[2:3], neural_rendering_resolution=16, noise_mode='const')
    assert torch.equal(one['image'], fl['image'][2:3]) and torch.equal(one['semantic'], fl['semantic'][2:3])      # CPU: frozen views are evaluated singly
    with pytest.raises(ValueError):
        views.render_views(G, ws[:2], cams, neural_rendering_resolution=16)


def test_edge_generator_gives_grey_label_frames_and_generate_video_writes_two_gifs(tmp_path):
    from PIL import Image
    from pix2pix3d_amd import views
    G = _small('edge2car')
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(8))
    p, pl = tmp_path / 'v.gif', tmp_path / 'v_label.gif'
    out = views.generate_video(G, ws, 'edge2car', str(p), str(pl), n_frames=4, views_per_step=3, neural_rendering_resolution=16)
    res = G.img_resolution
    assert tuple(out['image'].shape) == (4, res, res, 3) and tuple(out['label'].shape) == (4, res, res) and 'label_index' not in out
    for path in (p, pl):
        with Image.open(path) as im:
            assert im.n_frames == 4 and im.size == (res, res)
    s = views.generate_sample(G, ws, views.video_cameras(G, 'edge2car', 4)[1], str(tmp_path / 'c.png'), str(tmp_path / 'l.png'), neural_rendering_resolution=16)
    with Image.open(tmp_path / 'c.png') as im:
        assert np.array_equal(np.asarray(im), s['image'][0].numpy())
    with Image.open(tmp_path / 'l.png') as im:
        assert np.array_equal(np.asarray(im), s['label'][0].numpy())
