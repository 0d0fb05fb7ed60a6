"""pix2pix3d_amd.surface's second ray stage on the device: the occlusion kernel against the same counts composed over the point kernel
(integers: torch.equal), raster tiling and the limits, the public route against G.sample_mixed, the lit shade kernel against the CPU
formulation, render with lighting against its parts, and EditSession.geometry() with ambient occlusion."""
import math

import pytest
import torch

from model_cases import build_generator
from edit_cases import demo_pose, random_mask
from pix2pix3d_amd import _lib, surface
from pix2pix3d_amd.training.volumetric_rendering import renderer as rmod
from test_shape_gpu import _decoder
from test_surface_gpu import EPS, HALF_BOX, OPT, _generator_case, _point_sigma, _ray_max, _rays, _same_bytes, planes  # noqa: F401  (planes: the module's fixture)

pytestmark = pytest.mark.gpu

NEAR, FAR, CAST_STEPS, REFINE = 1.3, 2.8, 24, 5
REACH = 0.25


def _surface_points(planes, dec, side):
    """Two sets of side^2 points ON the level set of the test planes: the cast's hit positions (misses inactive), facing = -grad."""
    o, d = _rays(side)
    thr = float(torch.cat([_ray_max(_point_sigma(planes[n:n + 1] if planes.shape[0] > 1 else planes, dec), o[n], d[n], NEAR, FAR, CAST_STEPS, HALF_BOX)[0]
                           for n in range(2)]).median())
    hit, _, position, grad = rmod.fused_surface_cast(planes, dec, o, d, OPT, NEAR, FAR, CAST_STEPS, REFINE, thr, EPS, HALF_BOX)
    return position, -grad, hit


def _used(facing, active, dirs):
    """[P, K]: the definition's rule, three rounded products and two rounded sums."""
    dot = facing[:, None, 0] * dirs[None, :, 0]
    dot = dot + facing[:, None, 1] * dirs[None, :, 1]
    dot = dot + facing[:, None, 2] * dirs[None, :, 2]
    return (active != 0)[:, None] & (dot > 0)


def _pair_max(sigma_fn, origin, dirs, reach, steps, half_box):
    """[P, K]: per (point, direction) the largest in-box density among the ray's own samples (s_j and the points formed as the definition forms
    them; -inf where no sample is inside; a NaN density counts as -inf: it never blocks)."""
    dev = origin.device
    ds = torch.tensor(reach / steps, dtype=torch.float32, device=dev)
    s = torch.arange(1, steps + 1, dtype=torch.float32, device=dev) * ds
    p = origin[:, None, None, :] + s[None, None, :, None] * dirs[None, :, None, :]
    sig = sigma_fn(p.reshape(-1, 3)).reshape(p.shape[:3])
    inside = (p.abs() <= half_box).all(dim=-1) if half_box > 0 else torch.ones_like(sig, dtype=torch.bool)
    sig = torch.where(inside & ~torch.isnan(sig), sig, torch.full_like(sig, float('-inf')))
    return sig.max(dim=2).values


# ---- 1. the kernel equals the composition over the point kernel ------------------------------------------------------------------
@pytest.mark.parametrize('shared', [True, False], ids=['shared_planes', 'per_image'])
@pytest.mark.parametrize('nets', [1, 2])
def test_occlusion_equals_the_composition_over_the_point_kernel(hip_lib, planes, nets, shared):
    dec = _decoder(nets, seed=nets).cuda()
    used_planes = planes[:1] if shared else planes
    k, steps = 12, 6
    with torch.no_grad():
        origin, facing, active = _surface_points(used_planes, dec, 20)            # 2 x 400 points: 12.5 tiles per set
        fns = [_point_sigma(used_planes[0:1] if shared else used_planes[n:n + 1], dec) for n in range(2)]
        base = surface.sphere_directions(k).cuda()
        dirs = torch.stack([base, -base.flip(0)]).contiguous()                    # a direction table of its own for every set
        use = [_used(facing[n], active[n], dirs[n]) for n in range(2)]
        top = [_pair_max(fns[n], origin[n], dirs[n], REACH, steps, HALF_BOX) for n in range(2)]
        pairs = torch.cat([top[n][use[n]] for n in range(2)])
        thr = float(pairs[torch.isfinite(pairs)].median())                        # a used ray is blocked iff its largest in-box sample exceeds the threshold: about half are
        blocked = [use[n] & (top[n] > thr) for n in range(2)]
        want_total = torch.stack([use[n].sum(dim=1) for n in range(2)]).to(torch.uint8)
        want_open = torch.stack([(use[n] & ~blocked[n]).sum(dim=1) for n in range(2)]).to(torch.uint8)
        n0 = _lib.launch_count('render')
        open_, total = rmod.fused_surface_occlusion(used_planes, dec, origin, facing, active, dirs, OPT, REACH, steps, thr, HALF_BOX)
        torch.cuda.synchronize()
        assert _lib.launch_count('render') == n0 + 1
        ref = [surface.occlusion_rays(fns[n], origin[n], facing[n], active[n], dirs[n], REACH, steps, thr, half_box=HALF_BOX) for n in range(2)]
    n_used = int(sum(int(u.sum()) for u in use))
    share = sum(int(b.sum()) for b in blocked) / max(n_used, 1)
    mixed = int(((want_open > 0) & (want_open < want_total)).sum())
    print('active points', int(active.sum()), 'used pairs', n_used, 'blocked share', share, 'threshold', thr, 'points with 0 < open < total', mixed)
    assert 0.2 <= share <= 0.8
    assert mixed >= 100
    assert open_.dtype == torch.uint8 and total.dtype == torch.uint8 and tuple(open_.shape) == tuple(total.shape) == (2, 400)
    assert torch.equal(torch.stack([r[0] for r in ref]), want_open) and torch.equal(torch.stack([r[1] for r in ref]), want_total)
    assert torch.equal(total, want_total)
    assert torch.equal(open_, want_open)


@pytest.mark.parametrize('nets', [1, 2])
def test_planes_read_in_place_give_the_bytes_of_the_relayout_pass(hip_lib, nets):
    """csrc/render_host.h's one argument fill serves both layouts ``_plane_set_cl`` hands the density kernels: a channels-last [N, 96, H, W] tensor read
    in place through its strides, and the same values through the re-layout pass to [N][3][H][W][32]."""
    cl = (torch.randn([2, 96, 16, 16], generator=torch.Generator().manual_seed(23)) * 2).cuda().contiguous(memory_format=torch.channels_last)
    in_place = cl.view(2, 3, 32, 16, 16)
    copied = in_place.contiguous()
    assert rmod._plane_set_cl(in_place)[1] == (96 * 256, 32, 96) and rmod._plane_set_cl(copied)[1] == (0, 0, 0)
    dec = _decoder(nets, seed=nets).cuda()
    xs, ys, zs = (torch.linspace(-0.5, 0.5, n) for n in (5, 6, 7))                 # 210 points: six tiles and a partial one
    o, d = (t[:, :72].contiguous() for t in _rays(9))                              # 72 rays: two tiles and a quarter
    dirs = surface.sphere_directions(3).cuda()[None].expand(2, -1, -1).contiguous()
    with torch.no_grad():
        lattice = [rmod.fused_sample_lattice(p, dec, xs, ys, zs, OPT) for p in (in_place, copied)]
        assert tuple(lattice[0].shape) == (2, 5, 6, 7) and torch.equal(lattice[0], lattice[1])
        thr = float(lattice[1].flatten().quantile(0.75))
        for first in (2, 1):                                                       # per-set planes; set 0 shared over the two ray sets
            cast = [rmod.fused_surface_cast(p[:first], dec, o, d, OPT, NEAR, FAR, 8, 2, thr, EPS, HALF_BOX) for p in (in_place, copied)]
            assert all(_same_bytes(a, b) for a, b in zip(*cast))
            hit, _, position, grad = cast[1]
            assert bool(hit.any()) and not bool(hit.all())
            counts = [rmod.fused_surface_occlusion(p[:first], dec, position, -grad, hit, dirs, OPT, REACH, 4, thr, HALF_BOX) for p in (in_place, copied)]
            assert all(torch.equal(a, b) for a, b in zip(*counts))
            assert int(counts[1][1].sum()) > 0


# ---- 2. scheduling does not change a count; the limits -----------------------------------------------------------------------------
def test_raster_tiling_direction_counts_and_limits(hip_lib, planes):
    dec = _decoder(2, seed=2).cuda()
    steps = 6
    with torch.no_grad():
        origin, facing, active = _surface_points(planes, dec, 24)
        dirs12 = surface.sphere_directions(12).cuda()[None].expand(2, -1, -1).contiguous()
        probe = torch.cat([_pair_max(_point_sigma(planes[n:n + 1], dec), origin[n], dirs12[n], REACH, steps, HALF_BOX)[_used(facing[n], active[n], dirs12[n])]
                           for n in range(2)])
        thr = float(probe[torch.isfinite(probe)].median())
        tiled = rmod.fused_surface_occlusion(planes, dec, origin, facing, active, dirs12, OPT, REACH, steps, thr, HALF_BOX, raster_width=24)
        linear = rmod.fused_surface_occlusion(planes, dec, origin, facing, active, dirs12, OPT, REACH, steps, thr, HALF_BOX, raster_width=0)
        assert torch.equal(tiled[0], linear[0]) and torch.equal(tiled[1], linear[1])
        assert 0 < int((linear[0] < linear[1]).sum()) and 0 < int(((linear[0] == linear[1]) & (linear[1] > 0)).sum())
        # K = 1 and K = 255 on a 64-point set, against the definition over the point kernel
        o64, f64, a64 = origin[:, :64].contiguous(), facing[:, :64].contiguous(), active[:, :64].contiguous()
        for k in (1, 255):
            dirs = surface.sphere_directions(k).cuda()
            if k == 1:
                good = (a64[0] != 0) & torch.isfinite(f64[0]).all(dim=-1) & (f64[0].norm(dim=-1) > 0)
                dirs = torch.nn.functional.normalize(f64[0, good][:1], dim=-1)                  # a direction that the first point with a normal does use
            got = rmod.fused_surface_occlusion(planes, dec, o64, f64, a64, dirs[None].expand(2, -1, -1).contiguous(), OPT, REACH, 3, thr, HALF_BOX)
            ref = [surface.occlusion_rays(_point_sigma(planes[n:n + 1], dec), o64[n], f64[n], a64[n], dirs, REACH, 3, thr, half_box=HALF_BOX) for n in range(2)]
            print('K', k, 'largest total', int(got[1].max()), 'open sum', int(got[0].sum()), 'total sum', int(got[1].sum()))
            assert int(got[1].max()) >= (1 if k == 1 else 100)
            assert torch.equal(got[0], torch.stack([r[0] for r in ref])) and torch.equal(got[1], torch.stack([r[1] for r in ref]))
        # the wave-uniform exits: everything blocked at the first sample, nothing blocked at all, nothing to do
        count = torch.stack([_used(facing[n], active[n], dirs12[n]).sum(dim=1) for n in range(2)]).to(torch.uint8)
        low = rmod.fused_surface_occlusion(planes, dec, origin, facing, active, dirs12, OPT, REACH, steps, -1e30, 0.0)
        high = rmod.fused_surface_occlusion(planes, dec, origin, facing, active, dirs12, OPT, REACH, steps, 1e30, 0.0)
        idle = rmod.fused_surface_occlusion(planes, dec, origin, facing, torch.zeros_like(active), dirs12, OPT, REACH, steps, thr, HALF_BOX)
        torch.cuda.synchronize()
        assert int(count.max()) > 0
        assert torch.equal(low[1], count) and not bool(low[0].any())
        assert torch.equal(high[1], count) and torch.equal(high[0], count)
        assert not bool(idle[0].any()) and not bool(idle[1].any())
    n0 = _lib.launch_count()
    for k, s in ((0, steps), (256, steps), (12, 0), (12, 4097)):
        bad = torch.zeros([2, k, 3], device='cuda') if k != 12 else dirs12
        with pytest.raises(RuntimeError, match='directions'):
            rmod.fused_surface_occlusion(planes, dec, origin, facing, active, bad, OPT, REACH, s, thr, HALF_BOX)
    with pytest.raises(RuntimeError, match='raster_width'):
        rmod.fused_surface_occlusion(planes, dec, origin[:, :400].contiguous(), facing[:, :400].contiguous(), active[:, :400].contiguous(), dirs12, OPT, REACH,
                                     steps, thr, HALF_BOX, raster_width=20)
    assert _lib.launch_count() == n0


# ---- 3. the public route -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['seg2cat', 'edge2car'])
def test_occlusion_equals_occlusion_rays_over_sample_mixed(hip_lib, name):
    res, steps, refine, k, s = 32, 32, 4, 8, 6
    G, ws, cams, thr, fn, _, _ = _generator_case(name, res, 2, steps, seed=5)
    box = G.rendering_kwargs['box_warp']
    dirs = surface.sphere_directions(k)
    prev, rmod.fused_policy = rmod.fused_policy, 'require'
    try:
        hit = surface.cast(G, ws, cams, resolution=res, steps=steps, refine=refine, threshold=thr)
        n0 = _lib.launch_count('render')
        open_, total = surface.occlusion(G, ws, hit, dirs, box / 4, steps=s, threshold=thr)
        torch.cuda.synchronize()
        assert _lib.launch_count('render') > n0
        origin, facing, active = surface.occlusion_points(hit, box / 128)
        want = surface.occlusion_rays(fn, origin.reshape(-1, 3), facing.reshape(-1, 3), active.reshape(-1), dirs, box / 4, s, thr, half_box=box / 2)
    finally:
        rmod.fused_policy = prev
    share = float(hit.hit.float().mean())
    print(name, 'hit share', share, 'active', int(active.sum()), 'used pairs', int(want[1].sum()), 'open pairs', int(want[0].sum()))
    assert 0.05 < share < 0.95
    assert open_.is_cuda and open_.dtype == torch.uint8 and tuple(open_.shape) == tuple(total.shape) == (2, res, res)
    assert int(total.max()) > 0 and not bool(total[hit.hit == 0].any())
    assert torch.equal(total.reshape(-1), want[1])
    assert torch.equal(open_.reshape(-1), want[0])
    per_view = surface.occlusion(G, ws, hit, torch.stack([dirs, dirs]), box / 4, steps=s, threshold=thr)         # [V, K, 3] directions
    assert torch.equal(per_view[0], open_) and torch.equal(per_view[1], total)


def test_occlusion_fallback_follows_policy(hip_lib):
    G = build_generator('edge2car', 'cuda')
    ws = torch.zeros([1, G.backbone.num_ws, 512], device='cuda')
    hit = surface.SurfaceHit(torch.zeros([1, 8, 8], dtype=torch.uint8, device='cuda'), torch.zeros([1, 8, 8], device='cuda'),
                             torch.zeros([1, 8, 8, 3], device='cuda'), torch.zeros([1, 8, 8, 3], device='cuda'))
    rk = G.rendering_kwargs
    prev, rmod.fused_policy = rmod.fused_policy, 'require'
    try:
        G.rendering_kwargs = dict(rk, density_noise=1.0)
        with pytest.raises(RuntimeError, match='surface occlusion kernel required'):
            surface.occlusion(G, ws, hit, surface.sphere_directions(4), 0.25, steps=2)
    finally:
        G.rendering_kwargs = rk
        rmod.fused_policy = prev


# ---- 4. the lit shade, render, the session -------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cat_case():
    """(G, ws, cams, threshold, SurfaceHit) of seg2cat at 3 x 32^2: shared, never modified."""
    res = 32
    G, ws, cams, thr, _, _, _ = _generator_case('seg2cat', res, 3, 32, seed=6)
    return G, ws, cams, thr, surface.cast(G, ws, cams, resolution=res, steps=32, refine=4, threshold=thr)


def test_shade_lit_kernel_equals_the_cpu_formulation(hip_lib, cat_case):
    res = 32
    G, ws, cams, thr, hit = cat_case
    idx = hit.hit.reshape(-1).nonzero()[:, 0]
    assert len(idx) > 200
    grad = hit.grad.clone().reshape(-1, 3)
    grad[idx[0], 0], grad[idx[1], 2], grad[idx[2]] = float('inf'), float('nan'), 0.0
    grad[idx[3]] = torch.tensor([float('-inf'), 1.0, float('nan')], device='cuda')
    hit = hit._replace(grad=grad.reshape(hit.grad.shape))
    assert int((~torch.isfinite(hit.grad).all(dim=-1) & (hit.hit != 0)).sum()) >= 3
    host = surface.SurfaceHit(*(t.cpu() for t in hit))
    gen = torch.Generator().manual_seed(7)
    albedo = torch.randint(0, 256, [3, res, res, 3], generator=gen, dtype=torch.uint8)
    totals = [torch.randint(0, 9, [3, res, res], generator=gen, dtype=torch.uint8) for _ in range(2)]
    pairs = [((torch.rand([3, res, res], generator=gen) * (t.float() + 1)).floor().to(torch.uint8).minimum(t), t) for t in totals]
    lights = {'none': None, 'camera': surface.world_light((-0.5, -0.6, -0.6), cams[:, :16], 'camera'), 'world': surface.world_light((0.2, 1.0, 0.3), cams[:, :16], 'world')}
    dev_pair = lambda p: None if p is None else tuple(t.cuda() for t in p)
    for lname, light in lights.items():
        for alb in (None, albedo):
            for pname, ao, shadow in (('no pairs', None, None), ('ao', pairs[0], None), ('ao + shadow', pairs[0], pairs[1])):
                n0 = _lib.launch_count('aux')
                dev = surface.shade_lit(hit, cams[:, :16], None if alb is None else alb.cuda(), None if light is None else light.cuda(), dev_pair(ao),
                                        dev_pair(shadow), background=(10, 255, 0), ambient=0.25)
                torch.cuda.synchronize()
                assert _lib.launch_count('aux') > n0 and dev.is_cuda and dev.dtype == torch.uint8
                cpu = surface._shade_lit_cpu(host.hit, host.grad, alb, cams[:, :16].cpu(), light, ao, shadow, 0.25, (10, 255, 0))
                diff = int((dev.cpu() != cpu).any(dim=-1).sum())
                print('light', lname, 'albedo' if alb is not None else 'grey', pname, 'differing pixels', diff)
                assert diff == 0
                if light is None and ao is None:
                    assert torch.equal(dev, surface.shade(hit, cams[:, :16], None if alb is None else alb.cuda(), 'lambert', (10, 255, 0), 0.25))


def test_render_with_lighting_is_its_parts(hip_lib, cat_case):
    res = 32
    G, ws, cams, thr, hit = cat_case
    box = G.rendering_kwargs['box_warp']
    light = (-0.5, -0.6, -0.6)
    kw = dict(steps=32, refine=4, threshold=thr)
    frames = surface.render(G, ws, cams, res, ao=16, shadows=4, light=light, light_spread=0.1, **kw)
    assert frames.is_cuda and frames.dtype == torch.uint8 and tuple(frames.shape) == (3, res, res, 3)
    towards = surface.world_light(light, cams[:, :16], 'camera')
    ao = surface.occlusion(G, ws, hit, surface.sphere_directions(16), box / 4, steps=16, threshold=thr)
    shadow = surface.occlusion(G, ws, hit, surface.light_directions(towards, 4, 0.1), box * math.sqrt(3.0), steps=64, threshold=thr)
    assert torch.equal(frames, surface.shade_lit(hit, cams[:, :16], None, towards, ao, shadow))
    unlit = surface.render(G, ws, cams, res, **kw)
    drawn = hit.hit != 0
    print('drawn pixels', int(drawn.sum()), 'changed by the lighting', int((frames != unlit).any(dim=-1)[drawn].sum()),
          'ao open / total', int(ao[0].sum()), int(ao[1].sum()), 'shadow open / total', int(shadow[0].sum()), int(shadow[1].sum()))
    assert int((frames != unlit).any(dim=-1)[drawn].sum()) >= 1
    assert torch.equal(frames[~drawn], unlit[~drawn])


def test_session_geometry_with_ambient_occlusion(hip_lib):
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
    frame = s.geometry(resolution=32, ao=16, **kw)
    torch.cuda.synchronize()
    assert _lib.launch_count('conv') == conv and _lib.launch_count('render') == render + 2       # a camera move: the cast and ONE occlusion launch, no backbone
    assert s.geometry(resolution=32, ao=16, **kw) is frame and _lib.launch_count('render') == render + 2
    want = surface.render(G, s.encode(), s.camera, 32, planes=s._planes, ao=16, **kw)[0]
    assert frame.is_cuda and tuple(frame.shape) == (32, 32, 3) and torch.equal(frame, want)
    render = _lib.launch_count('render')
    other = s.geometry(resolution=32, ao=8, **kw)
    torch.cuda.synchronize()
    assert other is not frame and _lib.launch_count('render') == render + 2                       # another ao: recomputed
