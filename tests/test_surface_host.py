"""pix2pix3d_amd.surface without a GPU: the definition of the cast on analytic fields (sphere, two shells, the edge cases, the box
clip), the shade rule against Python loops, the generator path on CPU tensors and EditSession.geometry()'s caching."""
import math

import numpy as np
import pytest
import torch

from model_cases import build_generator
from edit_cases import Counters, demo_pose, random_mask
from pix2pix3d_amd import mesh, surface, views

R_SPHERE, NEAR, FAR, STEPS, REFINE = 0.3, 1.0, 3.0, 33, 6
DT = float(torch.tensor((FAR - NEAR) / (STEPS - 1), dtype=torch.float32))
ULP_FAR = float(np.spacing(np.float32(FAR)))


def _ortho_rays(n=16, span=0.4, distance=2.0):
    """n x n parallel rays along -z from the plane z = distance, on a grid spanning +-span."""
    a = torch.linspace(-span, span, n)
    yy, xx = torch.meshgrid(a, a, indexing='ij')
    o = torch.stack([xx, yy, torch.full_like(xx, distance)], -1).reshape(-1, 3)
    d = torch.tensor([0.0, 0.0, -1.0]).expand_as(o).contiguous()
    return o, d


def _sphere(radius, centre=(0.0, 0.0, 0.0)):
    c = torch.tensor(centre)
    return lambda p: radius - (p - c).norm(dim=-1)


@pytest.fixture(scope='module')
def sphere_cast():
    """(rays, SurfaceHit) of the analytic sphere: shared, never modified."""
    o, d = _ortho_rays()
    return o, d, surface.cast_rays(_sphere(R_SPHERE), o, d, NEAR, FAR, steps=STEPS, refine=REFINE, threshold=0.0)


# ---- 1. the definition on analytic fields ------------------------------------------------------------------------------------------
def test_sphere_hit_mask_and_depth(sphere_cast):
    o, d, out = sphere_cast
    assert out.hit.dtype == torch.uint8 and out.depth.dtype == torch.float32 and tuple(out.position.shape) == (256, 3) and tuple(out.grad.shape) == (256, 3)
    b = o[:, :2].double().norm(dim=-1)                                       # the ray's miss distance from the centre
    sure = (b - R_SPHERE).abs() > DT                                         # a chord longer than dt holds a sample; a ray further out than dt holds none
    want = b < R_SPHERE
    assert int(sure.sum()) > 150 and int((want & sure).sum()) > 50 and int((~want & sure).sum()) > 50
    assert torch.equal(out.hit[sure].bool(), want[sure])
    m = sure & want
    analytic = 2.0 - torch.sqrt(R_SPHERE ** 2 - b[m] ** 2)
    err = (out.depth[m].double() - analytic).abs()
    # six bisections leave an interval of dt / 64 that holds the crossing; the fp32 roundings of t, of the point and of the field move
    # the crossing itself by a few ulp of the largest depth
    bound = DT * 2.0 ** -REFINE + 4 * ULP_FAR
    print('depth error', float(err.max()), 'bound', bound)
    assert float(err.max()) <= bound
    assert torch.equal(out.position[m], (o + out.depth[:, None] * d)[m])


def test_sphere_gradient_direction(sphere_cast):
    o, d, out = sphere_cast
    eps = 1 / 256
    m = out.hit.bool() & ((o[:, :2].double().norm(dim=-1) - R_SPHERE).abs() > DT)
    p, n = out.position[m].double(), -out.grad[m].double()
    radial = p / p.norm(dim=-1, keepdim=True)
    angle = torch.atan2(torch.linalg.cross(n, radial).norm(dim=-1), (n * radial).sum(-1))
    # sigma = R - |x|: with u = p / |p| and h = eps / |p| the central difference along axis a is
    #   |p - eps e_a| - |p + eps e_a| = -2 eps u_a (1 - (h^2 / 2)(1 - u_a^2) + O(h^4)),
    # so -grad is 2 eps u plus a deviation of norm <= (h^2 / 2) 2 eps max|u_a (1 - u_a^2)| sqrt(3) < 2 eps h^2 / 3: an angle below (eps / R)^2
    # (|p| is within dt / 64 of R).  Each density carries an fp32 rounding error of about 2^-24 R (the norm, then an exact subtraction), a
    # difference of two 2^-23 R, against a gradient of length 2 eps: the cancellation term 2^-23 R / (2 eps).
    bound = (eps / R_SPHERE) ** 2 + 2.0 ** -23 * R_SPHERE / (2 * eps)
    print('gradient angle', float(angle.max()), 'bound', bound)
    assert int(m.sum()) > 50 and float(angle.max()) < bound


def test_two_shells_report_the_nearer():
    o, d = _ortho_rays(8, 0.1)
    near_shell, far_shell = _sphere(0.2, (0.0, 0.0, 0.5)), _sphere(0.2, (0.0, 0.0, -0.5))
    out = surface.cast_rays(lambda p: torch.maximum(near_shell(p), far_shell(p)), o, d, NEAR, FAR, steps=STEPS, refine=REFINE, threshold=0.0)
    b = o[:, :2].double().norm(dim=-1)
    analytic = 2.0 - 0.5 - torch.sqrt(0.2 ** 2 - b ** 2)
    assert bool(out.hit.all())
    assert float((out.depth.double() - analytic).abs().max()) <= DT * 2.0 ** -REFINE + 4 * ULP_FAR
    assert bool((out.position[:, 2] > 0.5).all())


def test_edge_cases():
    o, d = _ortho_rays(4, 0.1)
    ones = lambda p: torch.ones(p.shape[0])
    out = surface.cast_rays(ones, o, d, NEAR, FAR, steps=STEPS, refine=REFINE, threshold=0.0)
    assert bool(out.hit.all()) and torch.equal(out.depth, torch.full([16], NEAR))                 # sigma_0 above: depth == near exactly
    assert torch.equal(out.position, o + torch.tensor(NEAR) * d) and torch.equal(out.grad, torch.zeros(16, 3))
    for field in (lambda p: torch.full([p.shape[0]], float('nan')), lambda p: -torch.ones(p.shape[0])):
        out = surface.cast_rays(field, o, d, NEAR, FAR, steps=STEPS, refine=REFINE, threshold=0.0)   # a NaN field never hits; a miss is +inf / zeros
        assert not bool(out.hit.any()) and bool(torch.isposinf(out.depth).all())
        assert torch.equal(out.position, torch.zeros(16, 3)) and torch.equal(out.grad, torch.zeros(16, 3))
    out = surface.cast_rays(_sphere(R_SPHERE), o, d, NEAR, FAR, steps=STEPS, refine=0, threshold=0.0)       # refine = 0: t_i itself
    b = o[:, :2].double().norm(dim=-1)
    i = torch.ceil((2.0 - torch.sqrt(R_SPHERE ** 2 - b ** 2) - NEAR) / DT).to(torch.float32)
    assert bool(out.hit.all()) and torch.equal(out.depth, torch.tensor(NEAR) + i * torch.tensor(DT))
    for kw in (dict(steps=1), dict(steps=4097), dict(refine=25), dict(refine=-1)):
        with pytest.raises(ValueError):
            surface.cast_rays(ones, o, d, NEAR, FAR, **kw)


def test_box_clip():
    o, d = _ortho_rays(8, 0.4)
    ones = lambda p: torch.ones(p.shape[0])
    clipped = surface.cast_rays(ones, o, d, NEAR, FAR, steps=STEPS, refine=REFINE, threshold=0.0, half_box=0.25)
    inside = (o[:, :2].abs() <= 0.25).all(dim=-1)
    assert int(inside.sum()) > 0 and int((~inside).sum()) > 0
    assert torch.equal(clipped.hit.bool(), inside)
    # p.z = 2 - t_i with t_i = 1 + i / 16: the first sample with |p.z| <= 0.25 is i = 12, t = 1.75 (every bisection point lies outside)
    assert torch.equal(clipped.depth[inside], torch.full([int(inside.sum())], 1.75))
    free = surface.cast_rays(ones, o, d, NEAR, FAR, steps=STEPS, refine=REFINE, threshold=0.0)
    assert bool(free.hit.all()) and torch.equal(free.depth, torch.full([64], NEAR))


# ---- 2. the shade rule ---------------------------------------------------------------------------------------------------------------
def _shade_loops(hit, grad, albedo, cam, ambient, mode, background):
    """The rule of include/p3d_hip.h, pixel by pixel in Python floats (float64, one rounding per operation)."""
    h, w = hit.shape
    out = np.zeros([h, w, 3], np.uint8)
    amb = float(np.float32(ambient))
    f = [float(cam[j]) for j in (2, 6, 10)]
    for r in range(h):
        for c in range(w):
            if not hit[r, c]:
                out[r, c] = background
                continue
            g = [float(v) for v in grad[r, c]]
            if not all(math.isfinite(v) for v in g):
                g = [0.0, 0.0, 0.0]
            nn = g[0] * g[0]
            nn = nn + g[1] * g[1]
            nn = nn + g[2] * g[2]
            if mode == 'normal':
                n = math.sqrt(nn)
                for k in range(3):
                    u = -g[k] / n if n > 0 else 0.0
                    out[r, c, k] = min(max(math.floor((u * 0.5 + 0.5) * 255.0 + 0.5), 0), 255)
                continue
            ff = f[0] * f[0]
            ff = ff + f[1] * f[1]
            ff = ff + f[2] * f[2]
            dot = g[0] * f[0]
            dot = dot + g[1] * f[1]
            dot = dot + g[2] * f[2]
            den = math.sqrt(nn) * math.sqrt(ff)
            cosv = abs(dot) / den if den > 0 else 0.0
            s = amb + (1.0 - amb) * cosv
            for k in range(3):
                alb = float(albedo[r, c, k]) if albedo is not None else float(mesh.GREY)
                out[r, c, k] = min(max(math.floor(alb * s + 0.5), 0), 255)
    return out


@pytest.mark.parametrize('mode', ['lambert', 'normal'])
@pytest.mark.parametrize('with_albedo', [False, True])
def test_shade_equals_the_rule_written_as_loops(mode, with_albedo):
    g = torch.Generator().manual_seed(5)
    hit = (torch.rand([1, 5, 7], generator=g) > 0.25).to(torch.uint8)
    grad = torch.randn([1, 5, 7, 3], generator=g) * 3
    hit[0, 1, 2] = hit[0, 3, 4] = hit[0, 0, 0] = 1
    hit[0, 4, 6] = 0
    grad[0, 1, 2, 1] = float('inf')                                          # a non-finite gradient: the zero gradient
    grad[0, 3, 4] = 0.0                                                       # a zero gradient
    grad[0, 0, 0] = torch.tensor([0.0, 0.0, -2.0])                            # along the forward axis: cos = 1
    albedo = torch.randint(0, 256, [1, 5, 7, 3], generator=g, dtype=torch.uint8) if with_albedo else None
    cam = torch.eye(4)
    cam[:3, :3] = torch.linalg.qr(torch.randn([3, 3], generator=g)).Q
    cam[:3, 3] = torch.tensor([0.1, -0.2, 2.0])
    sh = surface.SurfaceHit(hit, torch.zeros(1, 5, 7), torch.zeros(1, 5, 7, 3), grad)
    got = surface.shade(sh, cam[None], albedo, mode=mode, background=(10, 255, 0), ambient=0.25)
    want = _shade_loops(hit[0].numpy(), grad[0].numpy(), None if albedo is None else albedo[0].numpy(), cam.reshape(-1).numpy(), 0.25, mode, (10, 255, 0))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 5, 7, 3)
    assert np.array_equal(got[0].numpy(), want)
    assert tuple(got[0, 4, 6].tolist()) == (10, 255, 0)
    if mode == 'normal':
        assert got[0, 1, 2].tolist() == [128, 128, 128] and got[0, 3, 4].tolist() == [128, 128, 128]
    elif not with_albedo:
        assert got[0, 1, 2].tolist() == [50, 50, 50] and got[0, 3, 4].tolist() == [50, 50, 50]        # ambient only: floor(200 * 0.25 + 0.5)
    with pytest.raises(ValueError):
        surface.shade(sh, cam[None], mode='phong')
    with pytest.raises(ValueError):
        surface.shade(sh, torch.eye(4).expand(2, 4, 4))


# ---- 3. a generator on the CPU -----------------------------------------------------------------------------------------------------
def _small():
    """tests/test_edit_host.py's small seg2cat generator: every density the fallback asks for is a backbone pass of G.sample_mixed, about thirty per test."""
    return build_generator('seg2cat', 'cpu', cbase=2048, cmax=32, depth=(6, 6), sr_num_fp16_res=0)


def test_cast_on_a_cpu_generator_equals_cast_rays_over_sample_mixed():
    G = _small()
    ws = torch.randn([1, G.backbone.num_ws, 512], generator=torch.Generator().manual_seed(2))
    cams = views.video_cameras(G, 'seg2cat', 2)
    rk = G.rendering_kwargs
    r, steps, refine = 8, 8, 3
    with torch.no_grad():
        ray_o, ray_d = G.ray_sampler(cams[:, :16].view(-1, 4, 4), cams[:, 16:25].view(-1, 3, 3), r)
        sigma_fn = lambda p: G.sample_mixed(p[None], None, ws, noise_mode='const')['sigma'].reshape(-1)
        mid = ray_o + 0.5 * (rk['ray_start'] + rk['ray_end']) * ray_d
        thr = float(sigma_fn(mid.reshape(-1, 3)).quantile(0.7))
    got = surface.cast(G, ws, cams, resolution=r, steps=steps, refine=refine, threshold=thr)
    want = surface.cast_rays(sigma_fn, ray_o.reshape(-1, 3), ray_d.reshape(-1, 3), rk['ray_start'], rk['ray_end'], steps=steps, refine=refine, threshold=thr,
                             eps=rk['box_warp'] / 256, half_box=rk['box_warp'] / 2)
    assert tuple(got.hit.shape) == (2, r, r) and tuple(got.depth.shape) == (2, r, r) and tuple(got.position.shape) == (2, r, r, 3) and tuple(got.grad.shape) == (2, r, r, 3)
    share = float(got.hit.float().mean())
    print('hit share', share)
    assert 0.0 < share < 1.0
    assert torch.equal(got.hit.reshape(-1), want.hit)
    for a, b in ((got.depth, want.depth), (got.position, want.position), (got.grad, want.grad)):
        assert a.numpy().tobytes() == b.numpy().tobytes()


def test_cast_argument_errors():
    G = _small()
    ws = torch.zeros([1, G.backbone.num_ws, 512])
    cams = views.video_cameras(G, 'seg2cat', 1)
    with pytest.raises(ValueError, match='one latent'):
        surface.cast(G, ws.expand(2, -1, -1), cams, resolution=8)
    with pytest.raises(ValueError, match='steps'):
        surface.cast(G, ws, cams, resolution=8, steps=1)
    with pytest.raises(ValueError, match='refine'):
        surface.cast(G, ws, cams, resolution=8, refine=25)
    with pytest.raises(ValueError, match='cameras'):
        surface.cast(G, ws, cams[:, :16], resolution=8)
    rk = G.rendering_kwargs
    try:
        G.rendering_kwargs = dict(rk, ray_start='auto', ray_end='auto')
        with pytest.raises(ValueError, match='near= and far='):
            surface.cast(G, ws, cams, resolution=8)
    finally:
        G.rendering_kwargs = rk
    with pytest.raises(ValueError, match='color'):
        surface.render(G, ws, cams, resolution=8, color='depth')


# ---- 4. EditSession.geometry() ---------------------------------------------------------------------------------------------------------
def test_session_geometry_runs_only_the_cast_and_keeps_its_frame(monkeypatch):
    from pix2pix3d_amd import edit
    G = _small()
    res = G.backbone.mapping.in_resolution
    s = edit.EditSession(G, seed=1, neural_rendering_resolution=16, hold_texture=False)
    casts = []
    real_cast = surface.cast
    monkeypatch.setattr(surface, 'cast', lambda *a, **k: casts.append(1) or real_cast(*a, **k))
    c = Counters(G)
    try:
        s.load(random_mask(1, res, res, 6, seed=4)[0], torch.from_numpy(demo_pose(G)))
        s.render()
        assert c.take() == (1, 1, 1)
        with torch.no_grad():
            pts = torch.rand([1, 512, 3], generator=torch.Generator().manual_seed(3)) - 0.5
            thr = float(G.renderer.run_model(surface._planes5(s._planes), G.decoder, pts, None, G.rendering_kwargs)['sigma'].median())
        kw = dict(resolution=8, steps=8, refine=2, threshold=thr)
        first = s.geometry(**kw)
        assert c.take() == (0, 0, 0) and len(casts) == 1                      # the planes were there: one cast, nothing else
        assert first.dtype == torch.uint8 and tuple(first.shape) == (8, 8, 3)
        assert s.geometry(**kw) is first and len(casts) == 1 and c.take() == (0, 0, 0)          # nothing changed: the kept frame, no cast
        want = surface.shade(real_cast(G, s.encode(), s.camera, planes=s._planes, **kw), s.camera[:, :16])[0]
        assert torch.equal(first, want) and 0 < int((first != 255).any(dim=-1).sum()) < 64
        s.set_camera(yaw=60, pitch=45, roll=3)
        turned = s.geometry(**kw)
        assert c.take() == (0, 0, 0) and len(casts) == 2                      # a camera move: one cast, neither the Encoder nor the backbone
        assert not torch.equal(turned, first)
        assert s.geometry(color='normal', **kw) is not turned and len(casts) == 3 and c.take() == (0, 0, 0)      # other arguments: another frame
        s.paint([(res // 4, res // 3, res // 2, res // 2, 35, 2)])
        s.geometry(**kw)
        assert c.take() == (1, 0, 1) and len(casts) == 4                      # an edit: Encoder and backbone once, then the cast
    finally:
        c.remove()
