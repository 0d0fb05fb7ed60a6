"""pix2pix3d_amd.surface's second ray stage without a GPU: the definition of the occlusion cast on an analytic scene (a ball resting on a
slab) and on its edge cases, the direction sets, the lit shade rule against the headlight rule, and render's defaults."""
import math

import pytest
import torch

from model_cases import build_generator
from pix2pix3d_amd import surface, views

BALL, SLAB_TOP, DENSE, THRESHOLD = 0.2, -0.2, 100.0, 50.0
UP = torch.tensor([[0.0, 0.0, 1.0]])


def _scene(p):
    """A ball of radius 0.2 about the origin resting on the slab z < -0.2: density 100 inside either, 0 outside."""
    inside = (p.norm(dim=-1) < BALL) | (p[:, 2] < SLAB_TOP)
    return torch.where(inside, torch.tensor(DENSE), torch.tensor(0.0))


def _floor_points(n=49, span=0.6):
    """n x n points on the slab's top, facing up: (origin, facing, active, |xy|)."""
    a = torch.linspace(-span, span, n)
    yy, xx = torch.meshgrid(a, a, indexing='ij')
    o = torch.stack([xx, yy, torch.full_like(xx, SLAB_TOP)], -1).reshape(-1, 3)
    return o, UP.expand_as(o).contiguous(), torch.ones(o.shape[0], dtype=torch.uint8), o[:, :2].double().norm(dim=-1)


@pytest.fixture(scope='module')
def floor():
    return _floor_points()


# ---- 1. the definition on an analytic scene ------------------------------------------------------------------------------------------
def test_shadow_of_the_ball(floor):
    o, f, act, rho = floor
    open_, total = surface.occlusion_rays(_scene, o, f, act, UP, reach=1.0, steps=64, threshold=THRESHOLD)
    assert open_.dtype == torch.uint8 and total.dtype == torch.uint8 and tuple(open_.shape) == tuple(total.shape) == (o.shape[0],)
    assert bool((total == 1).all())
    # under the ball the vertical chord is 2 sqrt(0.2^2 - 0.15^2) = 0.26 long at the least, seventeen sample spacings of 1 / 64
    under, clear = rho < 0.15, rho > 0.3
    assert int(under.sum()) > 50 and int(clear.sum()) > 1000
    assert bool((open_[under] == 0).all())
    assert bool((open_[clear] == 1).all())


def test_ambient_occlusion_near_the_contact(floor):
    o, f, act, rho = floor
    dirs = surface.sphere_directions(64)
    open_, total = surface.occlusion_rays(_scene, o, f, act, dirs, reach=0.25, steps=16, threshold=THRESHOLD)
    facing_count = int((dirs[:, 2] > 0).sum())
    assert 24 <= facing_count <= 40 and bool((total == facing_count).all())          # about half of the sphere faces any point
    # the ball's surface is sqrt(0.48^2 + 0.2^2) - 0.2 = 0.32 from a point at |xy| = 0.48: beyond the reach of 0.25; and no ray that goes up meets the slab
    far = rho > 0.48
    assert int(far.sum()) > 500 and bool((open_[far] == total[far]).all())
    # at 0.03 < |xy| < 0.12 the ball hangs less than 0.04 above the point: the rays that go up meet it within three sample spacings of 1 / 64
    near = (rho > 0.03) & (rho < 0.12)
    assert int(near.sum()) > 20 and bool((open_[near] < total[near]).all())
    assert bool((open_ <= total).all())


# ---- 2. the rules -------------------------------------------------------------------------------------------------------------------
def test_inactive_points_and_nan_facings(floor):
    o, f, act, rho = floor
    o, f, act = o[:64].clone(), f[:64].clone(), act[:64].clone()
    act[::2] = 0
    f[1, 0] = float('nan')
    f[3] = torch.tensor([0.0, 0.0, -1.0])                                              # faces down: neither direction below is used
    dirs = torch.tensor([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8]])
    open_, total = surface.occlusion_rays(lambda p: torch.zeros(p.shape[0]), o, f, act, dirs, reach=0.5, steps=4, threshold=THRESHOLD)
    assert bool((open_[::2] == 0).all()) and bool((total[::2] == 0).all())
    assert int(total[1]) == 0 and int(open_[1]) == 0 and int(total[3]) == 0
    rest = torch.ones(64, dtype=torch.bool)
    rest[::2], rest[1], rest[3] = False, False, False
    assert bool((total[rest] == 2).all()) and bool((open_[rest] == 2).all())


def test_a_nan_density_never_blocks(floor):
    o, f, act, _ = floor
    nan_field = lambda p: torch.full([p.shape[0]], float('nan'))
    open_, total = surface.occlusion_rays(nan_field, o[:32], f[:32], act[:32], UP, reach=0.5, steps=8, threshold=-1e30)
    assert bool((total == 1).all()) and bool((open_ == 1).all())
    dense = lambda p: torch.ones(p.shape[0])
    open_, total = surface.occlusion_rays(dense, o[:32], f[:32], act[:32], UP, reach=0.5, steps=8, threshold=0.0)
    assert bool((total == 1).all()) and bool((open_ == 0).all())


def test_box_clip_unblocks_a_blocker_outside_the_box():
    o = torch.tensor([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0]])
    f = UP.expand(2, 3).contiguous()
    act = torch.ones(2, dtype=torch.uint8)
    lid = lambda p: torch.where(p[:, 2] > 0.6, torch.tensor(DENSE), torch.tensor(0.0))        # a blocker beyond z = 0.6
    kw = dict(reach=1.0, steps=10, threshold=THRESHOLD)
    free = surface.occlusion_rays(lid, o, f, act, UP, **kw)
    clipped = surface.occlusion_rays(lid, o, f, act, UP, half_box=0.5, **kw)
    inside = surface.occlusion_rays(lid, o, f, act, UP, half_box=0.75, **kw)
    assert free[0].tolist() == [0, 0] and clipped[0].tolist() == [1, 1] and inside[0].tolist() == [0, 0]
    assert free[1].tolist() == clipped[1].tolist() == inside[1].tolist() == [1, 1]
    assert surface.occlusion_rays(lid, o, f, act, UP, half_box=0.0, **kw)[0].tolist() == [0, 0]      # half_box <= 0 clips nothing


def test_chunking_changes_nothing(floor):
    o, f, act, _ = floor
    o, f, act = o[::9], f[::9], act[::9].clone()
    act[5::7] = 0
    dirs = surface.sphere_directions(12)
    kw = dict(reach=0.25, steps=6, threshold=THRESHOLD, half_box=0.5)
    whole = surface.occlusion_rays(_scene, o, f, act, dirs, **kw)
    pieces = surface.occlusion_rays(_scene, o, f, act, dirs, max_bytes=37 * 1024, **kw)      # 37 points a chunk
    single = surface.occlusion_rays(_scene, o, f, act, dirs, max_bytes=1, **kw)              # one point a chunk
    assert 0 < int((whole[0] < whole[1]).sum()) < o.shape[0]
    assert torch.equal(whole[0], pieces[0]) and torch.equal(whole[1], pieces[1])
    assert torch.equal(whole[0], single[0]) and torch.equal(whole[1], single[1])


def test_argument_errors(floor):
    o, f, act, _ = floor
    zero = lambda p: torch.zeros(p.shape[0])
    for dirs, steps in ((torch.zeros(0, 3), 4), (surface.sphere_directions(256), 4), (UP, 0), (UP, 4097)):
        with pytest.raises(ValueError):
            surface.occlusion_rays(zero, o[:4], f[:4], act[:4], dirs, reach=0.5, steps=steps, threshold=0.0)
    with pytest.raises(ValueError):
        surface.occlusion_rays(zero, o[:4], f[:3], act[:4], UP, reach=0.5, steps=4, threshold=0.0)
    assert tuple(surface.occlusion_rays(zero, o[:0], f[:0], act[:0], UP, reach=0.5, steps=4, threshold=0.0)[0].shape) == (0,)


# ---- 3. the direction sets -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 8, 64, 255])
def test_sphere_directions(k):
    d = surface.sphere_directions(k)
    assert d.dtype == torch.float32 and tuple(d.shape) == (k, 3)
    assert float((d.double().norm(dim=-1) - 1).abs().max()) <= 1e-6
    assert torch.equal(d, surface.sphere_directions(k))
    if k >= 8:                                                                        # on the whole sphere: the set balances, and both hemispheres of any axis hold some
        assert float(d.double().mean(dim=0).norm()) < 1.5 / k ** 0.5
        assert all(0.3 * k < int((d[:, a] > 0).sum()) < 0.7 * k for a in range(3))


def test_light_directions():
    light = torch.nn.functional.normalize(torch.tensor([[-0.5, -0.6, -0.6], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]), dim=-1)
    one = surface.light_directions(light, 1, 0.3)
    assert one.dtype == torch.float32 and tuple(one.shape) == (3, 1, 3) and torch.equal(one[:, 0], light)      # samples = 1: the light itself
    assert tuple(surface.light_directions(light[0], 1).shape) == (1, 1, 3)
    spread = 0.1
    cone = surface.light_directions(light, 8, spread)
    assert cone.dtype == torch.float32 and tuple(cone.shape) == (3, 8, 3)
    assert float((cone.double().norm(dim=-1) - 1).abs().max()) <= 1e-6
    assert torch.equal(cone, surface.light_directions(light, 8, spread))
    angle = torch.acos((cone.double() * light.double()[:, None, :]).sum(-1).clamp(-1, 1))
    assert float(angle.max()) <= spread + 1e-6 and float(angle.max()) > 0.8 * spread      # inside the cone, and out to its rim
    assert float((cone.double().mean(dim=1) - light.double() * math.cos(spread / 2)).norm(dim=-1).max()) < 0.3 * spread      # about the axis
    tight = surface.light_directions(light, 4, 0.0)
    assert float((tight.double() - light.double()[:, None, :]).abs().max()) <= 1e-6
    with pytest.raises(ValueError):
        surface.light_directions(light, 0)


def test_world_light():
    cams = views.video_cameras(build_generator('seg2cat', 'cpu', cbase=2048, cmax=32, depth=(6, 6), sr_num_fp16_res=0), 'seg2cat', 3)
    cam = surface.world_light((-0.5, -0.6, -0.6), cams, 'camera')
    assert cam.dtype == torch.float32 and tuple(cam.shape) == (3, 3) and float((cam.double().norm(dim=-1) - 1).abs().max()) <= 1e-6
    rot = cams[:, :16].view(3, 4, 4)[:, :3, :3].double()
    want = rot @ torch.nn.functional.normalize(torch.tensor([-0.5, -0.6, -0.6], dtype=torch.float64), dim=0)
    assert float((cam.double() - want).abs().max()) < 1e-6 and not torch.equal(cam[0], cam[1])
    world = surface.world_light((0.0, 3.0, 0.0), cams, 'world')
    assert torch.equal(world, torch.tensor([[0.0, 1.0, 0.0]]).expand(3, 3))
    with pytest.raises(ValueError):
        surface.world_light((0.0, 0.0, 0.0), cams)
    with pytest.raises(ValueError):
        surface.world_light((0.0, 1.0, 0.0), cams, 'object')


# ---- 4. the lit shade rule ---------------------------------------------------------------------------------------------------------
def _shade_case(seed=5, v=2, h=9, w=11):
    g = torch.Generator().manual_seed(seed)
    hit = (torch.rand([v, h, w], generator=g) > 0.25).to(torch.uint8)
    grad = torch.randn([v, h, w, 3], generator=g) * 3
    hit[0, 1, 2] = hit[0, 3, 4] = hit[0, 0, 0] = hit[1, 2, 2] = hit[1, 5, 5] = 1
    hit[0, 4, 6] = 0
    grad[0, 1, 2, 1] = float('inf')
    grad[0, 3, 4] = 0.0
    grad[1, 2, 2, 0] = float('nan')
    grad[1, 5, 5] = torch.tensor([float('-inf'), 1.0, float('nan')])
    cams = torch.eye(4).repeat(v, 1, 1)
    for i in range(v):
        cams[i, :3, :3] = torch.linalg.qr(torch.randn([3, 3], generator=g)).Q
    albedo = torch.randint(0, 256, [v, h, w, 3], generator=g, dtype=torch.uint8)
    return surface.SurfaceHit(hit, torch.zeros(v, h, w), torch.zeros(v, h, w, 3), grad), cams.reshape(v, 16), albedo


@pytest.mark.parametrize('with_albedo', [False, True])
def test_shade_lit_with_nothing_optional_is_the_lambert_shade(with_albedo):
    sh, cams, albedo = _shade_case()
    alb = albedo if with_albedo else None
    want = surface._shade_cpu(sh.hit, sh.grad, alb, cams, 0.25, 'lambert', (10, 255, 0))
    got = surface._shade_lit_cpu(sh.hit, sh.grad, alb, cams, None, None, None, 0.25, (10, 255, 0))
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    assert torch.equal(surface.shade_lit(sh, cams, alb, background=(10, 255, 0), ambient=0.25), want)
    assert torch.equal(surface.shade_lit(sh, cams, alb, background=(10, 255, 0), ambient=0.25), surface.shade(sh, cams, alb, 'lambert', (10, 255, 0), 0.25))
    assert int(((sh.hit != 0) & ~torch.isfinite(sh.grad).all(dim=-1)).sum()) >= 3


def test_shade_lit_pairs_and_light():
    sh, cams, _ = _shade_case()
    v, h, w = sh.hit.shape
    g = torch.Generator().manual_seed(9)
    total = torch.randint(0, 9, [v, h, w], generator=g, dtype=torch.uint8)
    open_ = (torch.rand([v, h, w], generator=g) * (total.float() + 1)).floor().clamp(max=255).to(torch.uint8).minimum(total)
    base = surface.shade_lit(sh, cams, ambient=0.25)
    drawn = sh.hit != 0
    # ao_total == 0: ao = 1 — the frame without the pair, wherever the total is 0
    ao = surface.shade_lit(sh, cams, ao=(open_, total), ambient=0.25)
    none = drawn & (total == 0)
    assert int(none.sum()) > 5 and torch.equal(ao[none], base[none])
    full = drawn & (total > 0) & (open_ == total)
    assert int(full.sum()) > 5 and torch.equal(ao[full], base[full])
    assert bool((ao.int() <= base.int()).all()) and int((ao != base).sum()) > 0
    # sh_open == 0: exactly the ambient term, floor(200 * 0.25 + 0.5) = 50 on the grey albedo
    dark = surface.shade_lit(sh, cams, shadow=(torch.zeros_like(total), torch.ones_like(total)), ambient=0.25)
    assert bool((dark[drawn] == 50).all()) and bool((dark[~drawn] == 255).all())
    both = surface.shade_lit(sh, cams, ao=(torch.zeros_like(total), torch.ones_like(total)), shadow=(torch.zeros_like(total), torch.ones_like(total)), ambient=0.25)
    assert bool((both[drawn] == 0).all())
    # a light: the side that faces it is lit, the other side holds the ambient term only; a light along -g / |g| gives the full albedo
    light = torch.tensor([0.3, -0.5, 0.8])
    lit = surface.shade_lit(sh, cams, light=light, ambient=0.25)
    finite = torch.isfinite(sh.grad).all(dim=-1)
    away = drawn & finite & ((sh.grad.double() * light.double()).sum(-1) > 1e-9)
    assert int(away.sum()) > 10 and bool((lit[away] == 50).all())
    towards = drawn & finite & ((sh.grad.double() * light.double()).sum(-1) < -1e-3)
    assert int(towards.sum()) > 10 and bool((lit[towards] > 50).all())
    one = surface.SurfaceHit(torch.ones(1, 1, 1, dtype=torch.uint8), torch.zeros(1, 1, 1), torch.zeros(1, 1, 1, 3), torch.tensor([[[[0.0, 0.0, -2.0]]]]))
    assert surface.shade_lit(one, cams[:1], light=(0.0, 0.0, 5.0), ambient=0.25).reshape(-1).tolist() == [200, 200, 200]
    assert surface.shade_lit(one, cams[:1], light=(0.0, 0.0, 0.0), ambient=0.25).reshape(-1).tolist() == [50, 50, 50]          # |l| = 0: cos = 0
    per_view = surface.shade_lit(sh, cams, light=torch.stack([light, -light]), ambient=0.25)
    assert torch.equal(per_view[0], lit[0]) and not torch.equal(per_view[1], lit[1])
    with pytest.raises(ValueError):
        surface.shade_lit(sh, cams, ao=(open_, total[:1]))
    with pytest.raises(ValueError):
        surface.shade_lit(sh, cams, light=torch.zeros(5, 3))
    with pytest.raises(ValueError):
        surface.shade_lit(sh, torch.eye(4).expand(3, 4, 4))


# ---- 5. render -------------------------------------------------------------------------------------------------------------------------
def test_render_defaults_are_the_unlit_path_and_lighting_composes(monkeypatch):
    G = build_generator('seg2cat', 'cpu')
    ws = torch.randn([1, G.backbone.num_ws, 512], generator=torch.Generator().manual_seed(2))
    cams = views.video_cameras(G, 'seg2cat', 2)
    rk = G.rendering_kwargs
    r = 16
    with torch.no_grad():
        planes = G.backbone_planes(ws, noise_mode='const')
        ray_o, ray_d = G.ray_sampler(cams[:, :16].view(-1, 4, 4), cams[:, 16:25].view(-1, 3, 3), r)
        mid = ray_o + 0.5 * (rk['ray_start'] + rk['ray_end']) * ray_d
        thr = float(G.renderer.run_model(surface._planes5(planes), G.decoder, mid.reshape(1, -1, 3), None, rk)['sigma'].quantile(0.7))
    kw = dict(steps=8, refine=3, threshold=thr, planes=planes)
    lit_calls = []
    real_lit = surface.shade_lit
    monkeypatch.setattr(surface, 'shade_lit', lambda *a, **k: lit_calls.append(1) or real_lit(*a, **k))
    hit = surface.cast(G, ws, cams, resolution=r, **kw)
    frames = surface.render(G, ws, cams, resolution=r, **kw)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (2, r, r, 3)
    assert torch.equal(frames, surface.shade(hit, cams[:, :16])) and not lit_calls
    assert 0 < int(hit.hit.sum()) < 2 * r * r
    with pytest.raises(ValueError, match='light'):
        surface.render(G, ws, cams, resolution=r, shadows=1, **kw)
    # the lit frame is shade_lit over cast and the two occlusion calls; the CPU route is occlusion_rays over the planes' density
    light = (-0.5, -0.6, -0.6)
    got = surface.render(G, ws, cams, resolution=r, ao=6, shadows=2, light=light, light_spread=0.1, ao_steps=3, shadow_steps=4, **kw)
    assert len(lit_calls) == 1
    towards = surface.world_light(light, cams[:, :16], 'camera')
    box = rk['box_warp']
    ao = surface.occlusion(G, ws, hit, surface.sphere_directions(6), box / 4, steps=3, threshold=thr, planes=planes)
    shadow = surface.occlusion(G, ws, hit, surface.light_directions(towards, 2, 0.1), box * math.sqrt(3.0), steps=4, threshold=thr, planes=planes)
    assert torch.equal(got, real_lit(hit, cams[:, :16], None, towards, ao, shadow))
    assert tuple(ao[0].shape) == (2, r, r) and ao[0].dtype == torch.uint8
    drawn = hit.hit != 0
    assert bool((ao[1][~drawn] == 0).all()) and int(ao[1][drawn].max()) > 0 and torch.equal(got[~drawn], frames[~drawn])
    sigma_fn = lambda p: G.renderer.run_model(surface._planes5(planes), G.decoder, p[None], None, rk)['sigma'].reshape(-1)
    origin, facing, active = surface.occlusion_points(hit, box / 128)
    want = surface.occlusion_rays(sigma_fn, origin[1], facing[1], active[1], surface.sphere_directions(6), box / 4, 3, thr, half_box=box / 2)
    assert torch.equal(ao[0][1].reshape(-1), want[0]) and torch.equal(ao[1][1].reshape(-1), want[1])
