"""pix2pix3d_amd.surface on the device: the cast kernel against the same procedure composed over the point kernel (bit for bit), raster
tiling, the wave-uniform exits, the public cast against G.sample_mixed, the shade kernel against the CPU formulation, and
EditSession.geometry()."""
import pytest
import torch

from model_cases import build_generator
from edit_cases import demo_pose, random_mask
from pix2pix3d_amd import _lib, surface, views
from pix2pix3d_amd.training.volumetric_rendering import renderer as rmod
from test_shape_gpu import _decoder

pytestmark = pytest.mark.gpu

OPT = {'box_warp': 1.0}
HALF_BOX, EPS = 0.5, 1 / 256


def _same_bytes(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def _pinhole_set(origin, side, spread=0.3):
    """side x side rays from ``origin`` through a grid of +-spread about the box centre, normal to the axis the origin lies on."""
    o = torch.tensor(origin, dtype=torch.float32)
    a = torch.linspace(-spread, spread, side)
    u, v = torch.meshgrid(a, a, indexing='ij')
    axis = int(o.abs().argmax())
    target = torch.zeros(side, side, 3)
    target[..., (axis + 1) % 3], target[..., (axis + 2) % 3] = u, v
    d = torch.nn.functional.normalize(target.reshape(-1, 3) - o, dim=-1)
    return o.expand_as(d).contiguous(), d


def _rays(side):
    """Two sets of side^2 pinhole rays that cross the box [-0.5, 0.5]^3 from two sides: ([2, M, 3], [2, M, 3])."""
    sets = [_pinhole_set((0.0, 0.0, 2.0), side), _pinhole_set((2.0, 0.2, -0.1), side)]
    return torch.stack([s[0] for s in sets]).cuda(), torch.stack([s[1] for s in sets]).cuda()


def _ray_max(sigma_fn, o, d, near, far, steps, half_box):
    """Per ray the largest density among the march's own in-box samples (t_i and p formed as the cast forms them), and the samples."""
    dev = o.device
    dt = torch.tensor((far - near) / (steps - 1), dtype=torch.float32, device=dev)
    t = torch.tensor(near, dtype=torch.float32, device=dev) + torch.arange(steps, dtype=torch.float32, device=dev) * dt
    p = o[:, None, :] + t[None, :, None] * d[:, None, :]
    s = sigma_fn(p.reshape(-1, 3)).reshape(p.shape[:2])
    inside = (p.abs() <= half_box).all(dim=-1)
    s = s.masked_fill(~inside, float('-inf'))
    return s.max(dim=1).values, p, s


def _point_sigma(planes, dec):
    return lambda p: rmod.fused_sample_points(planes, dec, p[None].contiguous(), OPT)[1].reshape(-1)


@pytest.fixture(scope='module')
def planes():
    return (torch.randn([2, 3, 32, 64, 64], generator=torch.Generator().manual_seed(11)) * 2).cuda()


# ---- 1. the kernel equals the composition over the point kernel ------------------------------------------------------------------
@pytest.mark.parametrize('shared', [True, False], ids=['shared_planes', 'per_image'])
@pytest.mark.parametrize('nets', [1, 2])
def test_cast_equals_the_composition_over_the_point_kernel(hip_lib, planes, nets, shared):
    dec = _decoder(nets, seed=nets).cuda()
    near, far, steps, refine = 1.3, 2.8, 24, 5
    o, d = _rays(20)                                                          # 2 x 400 rays: 12.5 tiles per set
    used = planes[:1] if shared else planes
    fns = [_point_sigma(used[0:1] if shared else used[n:n + 1], dec) for n in range(2)]
    with torch.no_grad():
        probes = [_ray_max(fns[n], o[n], d[n], near, far, steps, HALF_BOX) for n in range(2)]
        ray_max = torch.cat([p[0] for p in probes])
        thr = float(ray_max.median())                                         # a ray hits iff its largest in-box sample exceeds the threshold: about half do
        # one ray that hits at i = 0: its first sample is the densest in-box sample of set 0
        best = int(probes[0][2].reshape(-1).argmax())
        p_best = probes[0][1].reshape(-1, 3)[best]
        d[0, 0] = torch.tensor([0.0, 0.0, -1.0], device='cuda')
        o[0, 0] = p_best + torch.tensor([0.0, 0.0, near], device='cuda')
        n0 = _lib.launch_count('render')
        hit, depth, position, grad = rmod.fused_surface_cast(used, dec, o, d, OPT, near, far, steps, refine, thr, EPS, HALF_BOX)
        torch.cuda.synchronize()
        assert _lib.launch_count('render') == n0 + 1
        ref = [surface.cast_rays(fns[n], o[n], d[n], near, far, steps=steps, refine=refine, threshold=thr, eps=EPS, half_box=HALF_BOX) for n in range(2)]
    ref = surface.SurfaceHit(*(torch.stack(t) for t in zip(*ref)))
    share = float(ref.hit.float().mean())
    print('hit share', share, 'threshold', thr, 'hits at i = 0', int((ref.depth == near).sum()), 'non-finite grads', int((~torch.isfinite(ref.grad)).sum()))
    assert 0.2 <= share <= 0.8
    assert bool(ref.hit[0, 0]) and float(ref.depth[0, 0]) == float(torch.tensor(near, dtype=torch.float32))
    assert int(((ref.hit == 1) & (ref.depth > near)).sum()) > 100               # and most hits went through the bisection
    assert hit.dtype == torch.uint8 and tuple(hit.shape) == (2, 400) and tuple(grad.shape) == (2, 400, 3)
    assert torch.equal(hit, ref.hit)
    assert _same_bytes(depth, ref.depth) and _same_bytes(position, ref.position) and _same_bytes(grad, ref.grad)


# ---- 2. scheduling does not change a byte; the wave-uniform exits --------------------------------------------------------------------
def test_raster_tiling_gives_identical_bytes(hip_lib, planes):
    dec = _decoder(2, seed=2).cuda()
    near, far, steps = 1.3, 2.8, 24
    o, d = _rays(24)
    with torch.no_grad():
        thr = float(torch.cat([_ray_max(_point_sigma(planes[n:n + 1], dec), o[n], d[n], near, far, steps, HALF_BOX)[0] for n in range(2)]).median())
        tiled = rmod.fused_surface_cast(planes, dec, o, d, OPT, near, far, steps, 5, thr, EPS, HALF_BOX, raster_width=24)
        linear = rmod.fused_surface_cast(planes, dec, o, d, OPT, near, far, steps, 5, thr, EPS, HALF_BOX, raster_width=0)
    share = float(linear[0].float().mean())
    print('hit share', share)
    assert 0.2 <= share <= 0.8
    assert torch.equal(tiled[0], linear[0]) and all(_same_bytes(a, b) for a, b in zip(tiled[1:], linear[1:]))
    with pytest.raises(RuntimeError, match='raster_width'):
        rmod.fused_surface_cast(planes, dec, o[:, :400], d[:, :400], OPT, near, far, steps, 5, thr, EPS, HALF_BOX, raster_width=20)
    for kw in (dict(steps=1), dict(steps=4097), dict(refine=25)):
        with pytest.raises(RuntimeError, match='steps'):
            rmod.fused_surface_cast(planes, dec, o, d, OPT, near, far, kw.get('steps', steps), kw.get('refine', 5), thr, EPS, HALF_BOX)


def test_wave_uniform_exits(hip_lib, planes):
    dec = _decoder(1, seed=1).cuda()
    near, far, steps = 1.3, 2.8, 24
    o, d = _rays(20)
    with torch.no_grad():
        low = rmod.fused_surface_cast(planes, dec, o, d, OPT, near, far, steps, 5, -1e30, EPS, 0.0)
        high = rmod.fused_surface_cast(planes, dec, o, d, OPT, near, far, steps, 5, 1e30, EPS, 0.0)
    torch.cuda.synchronize()
    assert bool(low[0].all()) and torch.equal(low[1], torch.full_like(low[1], near))
    assert torch.equal(low[2], o + torch.tensor(near, device='cuda') * d)
    assert not bool(high[0].any()) and bool(torch.isposinf(high[1]).all())
    assert torch.equal(high[2], torch.zeros_like(high[2])) and torch.equal(high[3], torch.zeros_like(high[3]))


# ---- 3. the public surface ---------------------------------------------------------------------------------------------------------
def _generator_case(name, resolution, n_views, steps, seed):
    """(G, ws, cameras, threshold): the threshold is the median over rays of the largest in-box density among the march's samples."""
    G = build_generator(name, 'cuda')
    ws = torch.randn([1, G.backbone.num_ws, 512], generator=torch.Generator().manual_seed(seed)).cuda()
    cams = views.video_cameras(G, name, n_views).cuda()
    rk = G.rendering_kwargs
    with torch.no_grad():
        o, d = G.ray_sampler(cams[:, :16].view(-1, 4, 4), cams[:, 16:25].view(-1, 3, 3), resolution)
        fn = lambda p: G.sample_mixed(p[None], None, ws, noise_mode='const')['sigma'].reshape(-1)
        ray_max = _ray_max(fn, o.reshape(-1, 3), d.reshape(-1, 3), rk['ray_start'], rk['ray_end'], steps, rk['box_warp'] / 2)[0]
    finite = ray_max[torch.isfinite(ray_max)]
    return G, ws, cams, float(finite.median()), fn, o, d


@pytest.mark.parametrize('name', ['seg2cat', 'edge2car'])
def test_cast_equals_cast_rays_over_sample_mixed(hip_lib, name):
    res, steps, refine = 32, 32, 4
    G, ws, cams, thr, fn, o, d = _generator_case(name, res, 2, steps, seed=5)
    rk = G.rendering_kwargs
    prev, rmod.fused_policy = rmod.fused_policy, 'require'
    try:
        n0 = _lib.launch_count('render')
        got = surface.cast(G, ws, cams, resolution=res, steps=steps, refine=refine, threshold=thr)
        torch.cuda.synchronize()
        assert _lib.launch_count('render') > n0
        want = surface.cast_rays(fn, o.reshape(-1, 3), d.reshape(-1, 3), rk['ray_start'], rk['ray_end'], steps=steps, refine=refine, threshold=thr,
                                 eps=rk['box_warp'] / 256, half_box=rk['box_warp'] / 2)
    finally:
        rmod.fused_policy = prev
    share = float(got.hit.float().mean())
    print(name, 'hit share', share, 'threshold', thr)
    assert 0.05 < share < 0.95
    assert got.hit.is_cuda and tuple(got.hit.shape) == (2, res, res) and tuple(got.grad.shape) == (2, res, res, 3)
    assert torch.equal(got.hit.reshape(-1), want.hit)
    assert _same_bytes(got.depth, want.depth) and _same_bytes(got.position, want.position) and _same_bytes(got.grad, want.grad)


def test_cast_fallback_follows_policy(hip_lib):
    G = build_generator('edge2car', 'cuda')
    ws = torch.zeros([1, G.backbone.num_ws, 512], device='cuda')
    cams = views.video_cameras(G, 'edge2car', 1).cuda()
    rk = G.rendering_kwargs
    prev, rmod.fused_policy = rmod.fused_policy, 'require'
    try:
        G.rendering_kwargs = dict(rk, density_noise=1.0)
        with pytest.raises(RuntimeError, match='surface cast kernel required'):
            surface.cast(G, ws, cams, resolution=8, steps=8)
    finally:
        G.rendering_kwargs = rk
        rmod.fused_policy = prev


def test_shade_kernel_equals_the_cpu_formulation(hip_lib):
    res = 32
    G, ws, cams, thr, _, _, _ = _generator_case('seg2cat', res, 3, 32, seed=6)
    hit = surface.cast(G, ws, cams, resolution=res, steps=32, refine=4, threshold=thr)
    # the rule for a gradient that is not finite, and for a zero one, on pixels that are hits
    idx = hit.hit.reshape(-1).nonzero()[:, 0]
    assert len(idx) > 200
    grad = hit.grad.clone().reshape(-1, 3)
    grad[idx[0], 0], grad[idx[1], 2], grad[idx[2]] = float('inf'), float('nan'), 0.0
    grad[idx[3]] = torch.tensor([float('-inf'), 1.0, float('nan')], device='cuda')
    hit = hit._replace(grad=grad.reshape(hit.grad.shape))
    bad = int((~torch.isfinite(hit.grad).all(dim=-1) & (hit.hit != 0)).sum())
    print('hit pixels', len(idx), 'of them with a non-finite gradient', bad)
    assert bad >= 3
    host = surface.SurfaceHit(*(t.cpu() for t in hit))
    albedo = torch.randint(0, 256, [3, res, res, 3], generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
    for mode, alb in (('lambert', None), ('normal', None), ('lambert', albedo)):
        n0 = _lib.launch_count('aux')
        dev = surface.shade(hit, cams[:, :16], None if alb is None else alb.cuda(), mode=mode, background=(10, 255, 0), ambient=0.25)
        torch.cuda.synchronize()
        assert _lib.launch_count('aux') > n0 and dev.is_cuda and dev.dtype == torch.uint8
        cpu = surface.shade(host, cams[:, :16].cpu(), alb, mode=mode, background=(10, 255, 0), ambient=0.25)
        diff = int((dev.cpu() != cpu).any(dim=-1).sum())
        print(mode, 'albedo' if alb is not None else 'grey', 'differing pixels', diff)
        assert diff == 0
    frames = surface.render(G, ws, cams, resolution=res, steps=32, refine=4, threshold=thr)
    assert tuple(frames.shape) == (3, res, res, 3) and frames.is_cuda and 0 < int((frames != 255).any(dim=-1).sum()) < 3 * res * res


def test_session_geometry_on_the_device(hip_lib):
    from pix2pix3d_amd import edit
    G = build_generator('seg2cat', 'cuda')
    res = G.backbone.mapping.in_resolution
    s = edit.EditSession(G, seed=1)
    s.load(random_mask(1, res, res, 6, seed=4)[0], torch.from_numpy(demo_pose(G)))
    s.render()
    with torch.no_grad():
        pts = (torch.rand([1, 4096, 3], generator=torch.Generator().manual_seed(3)) - 0.5).cuda()
        thr = float(rmod.fused_sample_points(surface._planes5(s._planes), G.decoder, pts, G.rendering_kwargs)[1].quantile(0.9))
    kw = dict(steps=32, refine=4, threshold=thr)
    s.set_camera(yaw=30, pitch=50)
    torch.cuda.synchronize()
    conv, render = _lib.launch_count('conv'), _lib.launch_count('render')
    frame = s.geometry(resolution=32, **kw)
    torch.cuda.synchronize()
    assert _lib.launch_count('conv') == conv and _lib.launch_count('render') == render + 1      # a camera move: one cast launch, no Encoder, no backbone
    assert s.geometry(resolution=32, **kw) is frame and _lib.launch_count('render') == render + 1
    want = surface.render(G, s.encode(), s.camera, 32, planes=s._planes, **kw)[0]
    print('drawn pixels', int((frame != 255).any(dim=-1).sum()))
    assert frame.is_cuda and tuple(frame.shape) == (32, 32, 3) and torch.equal(frame, want)
