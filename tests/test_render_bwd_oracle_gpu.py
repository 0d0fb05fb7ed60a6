"""Fused renderer backward (csrc/render_bwd.hip: p3d_render_backward, p3d_sample_points_backward) against fp64 autograd through
oracle.render_oracle.render_given_depths / sample_points_t, on seeded synthetic cases at the sizes where the kernel's work split differs
from the recorded golden cases: several 32-sample tiles per ray, tail tiles (S % 32 != 0), waves that take >= 8 tiles across many rays
and across image boundaries, ray counts that are not a square, the channels-last in-place plane read, and the point queries'
grid-stride second round.

The depths are the kernel's own (the tape, ``fused_render_backward(..., debug=True)[2][..., 0]``): importance depths are constants of the
backward (renderer.py:198, 211), so this takes the sampler out of the comparison (its bins are pinned by test_render_gpu.py).  The reference
gradients are fp64 autograd on the device through ATen; nothing here reads the reference project.

What is compared, each with its own normalisation (conftest.rel_err = max|a - b| / max|b|):
  * plane gradients per (image, plane) slice, normalised by that slice's own max: a wrong contribution confined to one image or plane
    shows even when another slice holds the global max;
  * texels farther than one texel from every tap of the oracle's sample coordinates must be exactly 0 (a scatter into the wrong image,
    plane or texel);
  * every decoder parameter separately (W1, b1, W2, b2 of each net, decoder.parameters() order);
  * the tape: colour weight (w[k-1] + w[k]) / 2 and dL/dsigma of every sample, against the oracle's weights and autograd.
Bounds: about 3x the worst error measured on an MI355X over two runs (recorded by conftest.record_error), all under
the 2e-4 ceiling.  The kernel's products are exact fp32 (mfma_f32_32x32x2f32) and its sums fp32 atomics: a few fp32 ulps amplified by the
sums, ~1e-5.
  * planes (per slice)        4e-5    worst 1.2e-5 (the empty-space case; 8.6e-6 elsewhere)
  * decoder (per parameter)   2.5e-5  worst 7.9e-6
      empty-space case        1.2e-4  worst 4.1e-5: most of its samples have alpha = 1 - exp(-x) with x ~ 1e-4 .. 1e-8, where fp32 cancels
                                      (absolute error ~6e-8, as in the reference's own fp32 ray marcher) and the kernel's log(1 + exp(s))
                                      rounds the density of sigma < -17 to 0; the decoder sums see all of those samples, the slices of
                                      the planes mostly the dense pockets.
  * tape (weight, dL/dsigma)  6e-5    worst 2.1e-5 (dL/dsigma of the saturated case: x ~ 27 per coarse interval); 7.9e-6 elsewhere
  * points (planes, decoder)  1.5e-5  worst 4.8e-6
"""
import numpy as np
import pytest
import torch

from conftest import record_error

pytestmark = pytest.mark.gpu

F64 = torch.float64
K_FOCAL = 4.2647                               # the FFHQ-style intrinsics of the training configs (normalised focal length)

# bounds (see the module docstring)
B_PLANES = 4e-5
B_DEC = 2.5e-5
B_DEC_EMPTY = 1.2e-4
B_TAPE = 6e-5
B_POINTS = 1.5e-5


# ---------------------------------------------------------------------------------------------------------------------------------------
# builders

def _decoder(nets, sem_sigmoid, lr_mul, seed, sigma_gain=None, sigma_zero=None):
    """A decoder module of this package with seeded weights, distinct per net.  With ``sigma_gain`` the density row of the density net
    (the label net with two nets) is made zero-mean and scaled, and its bias set so that sigma = ``sigma_zero`` where the features are 0
    (outside the box): sigma then swings with the features instead of sitting near a constant, which makes empty (sigma << 0) and
    saturated (alpha == 1 in fp32) stretches inside the box, behind an empty approach."""
    from pix2pix3d_amd.training.triplane import OSGDecoder
    from pix2pix3d_amd.training.triplane_cond import OSGDecoder_semantic_lateSeparate
    opts = {'decoder_lr_mul': lr_mul, 'decoder_output_dim': 32}
    dec = OSGDecoder(32, opts) if nets == 1 else OSGDecoder_semantic_lateSeparate(32, dict(opts, sigmoid=sem_sigmoid, semantic_channels=6))
    g = torch.Generator().manual_seed(seed)
    seqs = [dec.net] if nets == 1 else [dec.net, dec.net_semantic]
    with torch.no_grad():
        for seq in seqs:                                   # effective weights ~ N(0, 1/fan_in), biases ~ N(0, 0.3^2) (raw values / lr_mul)
            for fc in (seq[0], seq[2]):
                fc.weight.copy_(torch.randn(fc.weight.shape, generator=g) / lr_mul)
                fc.bias.copy_(0.3 * torch.randn(fc.bias.shape, generator=g) / lr_mul)
        if sigma_gain is not None:
            fc1, fc2 = seqs[-1][0], seqs[-1][2]
            row = fc2.weight[0]
            fc2.weight[0] = (row - row.mean()) * sigma_gain
            h0 = torch.nn.functional.softplus(fc1.bias * lr_mul)                 # the hidden layer at zero features
            fc2.bias[0] = (sigma_zero - float(fc2.weight[0] @ h0) * lr_mul / 8) / lr_mul
    return dec.cuda().requires_grad_(True)


def _cameras(n, seed):
    """n cameras on a sphere of radius 2.7 looking at the origin (camera z = viewing direction, as ray_sampler.py lifts pixels to z = 1)."""
    g = torch.Generator().manual_seed(seed)
    c2w = torch.zeros(n, 4, 4)
    for i in range(n):
        yaw, pitch = (torch.rand(2, generator=g) - 0.5) * torch.tensor([2.4, 0.8])
        pos = 2.7 * torch.stack([torch.sin(yaw) * torch.cos(pitch), torch.sin(pitch), torch.cos(yaw) * torch.cos(pitch)])
        fwd = -pos / pos.norm()
        right = torch.linalg.cross(torch.tensor([0., 1., 0.]), fwd)
        right = right / right.norm()
        up = torch.linalg.cross(fwd, right)
        c2w[i, :3, 0], c2w[i, :3, 1], c2w[i, :3, 2], c2w[i, :3, 3], c2w[i, 3, 3] = right, up, fwd, pos, 1.
    return c2w


def _rays(n, m, seed):
    """[N, M, 3] origins / directions: the first M rays of the smallest square image with >= M pixels."""
    from pix2pix3d_amd.training.volumetric_rendering.ray_sampler import RaySampler
    r = int(np.ceil(np.sqrt(m)))
    K = torch.tensor([[K_FOCAL, 0, 0.5], [0, K_FOCAL, 0.5], [0, 0, 1]]).repeat(n, 1, 1)
    o, d = RaySampler()(_cameras(n, seed).cuda(), K.cuda(), r)
    return o[:, :m].contiguous(), d[:, :m].contiguous()


def _planes(n, h, w, seed, channels_last=False):
    g = torch.Generator(device='cuda').manual_seed(seed)
    if channels_last:                                      # a channels-last backbone output [N,96,H,W] viewed as [N,3,32,H,W]: read in place
        x = (0.5 * torch.randn(n, 96, h, w, device='cuda', generator=g)).contiguous(memory_format=torch.channels_last)
        return x.view(n, 3, 32, h, w)
    return 0.5 * torch.randn(n, 3, 32, h, w, device='cuda', generator=g)


def _dec64(dec):
    """fp64 leaf copies of the decoder parameters (decoder.parameters() order) and the oracle's dict view of them."""
    leaves, d = [], {}
    for name, p in dec.named_parameters():
        t = p.detach().to(F64).requires_grad_(True)
        leaves.append(t)
        net, layer, kind = name.split('.')
        d[('w' if kind == 'weight' else 'b') + ('1' if layer == '0' else '2') + ('s' if net == 'net_semantic' else '')] = t
    d['lr_mul'] = float(dec.net[0].bias_gain)
    d['semantic_sigmoid'] = bool(getattr(dec, 'semantic_sigmoid', False))
    return leaves, d


# ---------------------------------------------------------------------------------------------------------------------------------------
# checks

def _touched(uv, h, w):
    """[N,3,H,W] bool: texels within one texel of a bilinear tap (align_corners=False) of some coordinate in uv [N,3,P,2]."""
    n, k = uv.shape[:2]
    ix = ((uv[..., 0] + 1) * w - 1) / 2
    iy = ((uv[..., 1] + 1) * h - 1) / 2
    x0 = torch.floor(ix).clamp(-3, w + 1).long() + 3           # padded by 3: out-of-range taps land outside the crop even after dilation
    y0 = torch.floor(iy).clamp(-3, h + 1).long() + 3
    hit = torch.zeros(n * k, (h + 6) * (w + 6), device=uv.device)
    for dy in (0, 1):
        for dx in (0, 1):
            hit.scatter_(1, ((y0 + dy) * (w + 6) + x0 + dx).reshape(n * k, -1), 1.0)
    hit = torch.nn.functional.max_pool2d(hit.reshape(n * k, 1, h + 6, w + 6), 3, 1, 1)
    return hit[:, 0, 3:h + 3, 3:w + 3].reshape(n, k, h, w) > 0


def _slice_errs(gp, ref):
    """rel_err of every (image, plane) slice [32, H, W], normalised by the slice's own max; slices whose reference is all zero must be zero."""
    a, b = gp.detach().to(F64), ref.detach()
    num = (a - b).abs().amax(dim=(2, 3, 4))
    den = b.abs().amax(dim=(2, 3, 4))
    zero = den == 0
    assert not bool(zero.all())
    if bool(zero.any()):
        assert float(a.abs().amax(dim=(2, 3, 4))[zero].max()) == 0.0, 'gradient on a slice the oracle leaves at 0'
    return (num[~zero] / den[~zero])


def _rel(a, b):
    a, b = a.detach().to(F64), b.detach().to(F64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _check_planes(tag, gp, ref, uv, bound):
    assert gp.shape == ref.shape and bool(torch.isfinite(gp).all())
    errs = _slice_errs(gp, ref)
    worst = float(errs.max())
    record_error(tag + '.planes', worst)
    assert worst < bound, f'plane gradient, worst (image, plane) slice: {worst:.3e} (per slice: {errs.cpu().numpy()})'
    n, k, c, h, w = ref.shape
    far = ~_touched(uv, h, w)
    assert int(far.sum()) > 0, 'case does not leave any texel untouched: pick larger planes'
    stray = gp.detach().permute(0, 1, 3, 4, 2)[far]
    assert float(stray.abs().max()) == 0.0, f'{int((stray != 0).any(-1).sum())} texels no sample touches got a gradient'


def _check_decoder(tag, dec, gd, ref, bound):
    names = [k for k, _ in dec.named_parameters()]
    assert len(gd) == len(ref) == len(names)
    worst = {}
    for name, a, b in zip(names, gd, ref):
        assert a is not None and a.shape == b.shape, name
        assert float(b.abs().max()) > 0, name
        e = _rel(a, b)
        net = name.split('.')[0]
        worst[net] = max(worst.get(net, 0.0), e)
        assert e < bound, f'decoder gradient {name}: {e:.3e}'
    for net, e in worst.items():
        record_error(f'{tag}.dec_{net}', e)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fused render backward

# nets (1 OSG / 2 late-separate), sem: semantic_sigmoid, (sc, sf), n images x m rays, plane (H, W), lr: decoder lr_mul, cl: channels-last
# planes read in place, gw: a wsum gradient, opts: rendering options beyond the defaults, sig: (sigma_gain, sigma_bias) of the density row
RAY_CASES = {
    # training sample counts, 3 tiles per ray; 2 x 64^2 rays -> tpw = 24576 / 2048 = 12: a wave crosses 4 rays, the last waves straddle images
    'osg_48+48_tpw12': dict(nets=1, sc=48, sf=48, n=2, m=64 * 64, hw=(72, 56), lr=1.0, gw=True),
    'seg_48+48_tpw12_cl': dict(nets=2, sem=False, sc=48, sf=48, n=2, m=64 * 64, hw=(88, 120), lr=0.7, cl=True, gw=False),
    # maximum: 4 tiles per ray, tpw = 4, white background
    'segsig_64+64_white': dict(nets=2, sem=True, sc=64, sf=64, n=1, m=48 * 48, hw=(100, 60), lr=0.5, gw=True, opts=dict(white_back=True)),
    # S = 63: 2 tiles, tail of 31; 3001 rays per image (not a square): the last block and wave are partial, waves straddle images (tpw 5)
    'seg_33+30_tail31_3001': dict(nets=2, sem=False, sc=33, sf=30, n=2, m=3001, hw=(56, 88), lr=1.0, gw=True),
    # S = 37: 2 tiles, tail of 5; disparity-space stratified sampling
    'osg_20+17_tail5_disparity': dict(nets=1, sc=20, sf=17, n=1, m=40 * 40, hw=(40, 24), lr=2.0, gw=False,
                                      opts=dict(disparity_space_sampling=True)),
    # S = 65: 3 tiles, tail of 1; per-ray 'auto' limits from the box
    'segsig_64+1_tail1_auto': dict(nets=2, sem=True, sc=64, sf=1, n=2, m=30 * 30, hw=(64, 48), lr=1.0, gw=True,
                                   opts=dict(ray_start='auto', ray_end='auto')),
    # minimum sample counts, 3 images x 500 rays (not a square), channels-last planes
    'osg_4+1_min_500': dict(nets=1, sc=4, sf=1, n=3, m=500, hw=(30, 20), lr=1.0, gw=True, cl=True),
    # box_warp 0.55: a share of the samples falls outside [-1, 1] (zero-padded taps)
    'seg_24+24_outside_box': dict(nets=2, sem=False, sc=24, sf=24, n=2, m=32 * 32, hw=(48, 36), lr=1.0, gw=True, opts=dict(box_warp=0.55)),
    # empty space: sigma << 0 over most of the volume (many rays with wsum ~ 0), dense pockets elsewhere
    'osg_32+32_empty': dict(nets=1, sc=32, sf=32, n=2, m=24 * 24, hw=(40, 40), lr=1.0, gw=True, sig=(150.0, -32.0)),
    # saturated density: sigma ~ 800 everywhere, so every coarse interval has alpha == 1 in fp32 and 1 - alpha + 1e-10 is the back-to-front
    # sweep's divisor; the importance samples split the first interval into a steep but resolved fall of T.  (A saturation driven by large
    # feature-dependent swings of sigma instead, ~10^4 from a cancelling sum, carries the fp32 rounding of sigma, ~1e-3 absolute, into
    # exp(-sigma delta): 4e-4 measured, the conditioning of the case and not the kernel.)
    'segsig_32+32_saturated': dict(nets=2, sem=True, sc=32, sf=32, n=2, m=24 * 24, hw=(40, 40), lr=1.0, gw=True, sig=(30.0, 800.0)),
}


def _run_ray_case(name):
    from pix2pix3d_amd.training.volumetric_rendering import renderer as R
    from oracle import render_oracle as RO
    cfg = RAY_CASES[name]
    seed = sorted(RAY_CASES).index(name)
    nets, n, m, (h, w) = cfg['nets'], cfg['n'], cfg['m'], cfg['hw']
    sc, sf = cfg['sc'], cfg['sf']
    opt = dict(depth_resolution=sc, depth_resolution_importance=sf, ray_start=2.25, ray_end=3.3, box_warp=1.0, white_back=False,
               disparity_space_sampling=False, clamp_mode='softplus')
    opt.update(cfg.get('opts', {}))
    dec = _decoder(nets, cfg.get('sem', False), cfg['lr'], 100 + seed, *cfg.get('sig', (None, None)))
    planes = _planes(n, h, w, 200 + seed, cfg.get('cl', False))
    o, d = _rays(n, m, 300 + seed)
    torch.manual_seed(400 + seed)
    u_c = torch.rand(n, m, sc, device='cuda')
    u_f = torch.rand(n * m, sf, device='cuda')
    g_feat = torch.randn(n, m, 32 * nets, device='cuda')
    g_w = torch.randn(n, m, 1, device='cuda') if cfg['gw'] else None
    t0 = t1 = None
    if opt['ray_start'] == 'auto':
        t0, t1 = R.ImportanceRenderer()._ray_limits(o, d, opt)
    gp, gd, tape = R.fused_render_backward(planes, dec, o, d, opt, u_c, u_f, t0, t1, g_feat, g_w, debug=True)
    torch.cuda.synchronize()

    leaves, d64 = _dec64(dec)
    pl64 = planes.detach().to(F64).contiguous().requires_grad_(True)
    z = tape[..., 0].to(F64)
    assert bool((z[:, 1:] >= z[:, :-1]).all()), 'tape depths not sorted'
    out = RO.render_given_depths(pl64, d64, o, d, z, opt['box_warp'], bool(opt['white_back']))
    loss = (out['feat'] * g_feat.to(F64)).sum() + (0.0 if g_w is None else (out['wsum'] * g_w.to(F64).reshape(n, m)).sum())
    grads = torch.autograd.grad(loss, [pl64, out['sigmas']] + leaves)
    ref_p, ref_dsig, ref_dec = grads[0], grads[1], list(grads[2:])
    return dict(cfg=cfg, opt=opt, dec=dec, gp=gp, gd=gd, tape=tape, out=out, ref_p=ref_p, ref_dsig=ref_dsig, ref_dec=ref_dec)


@pytest.fixture(scope='module')
def ray_case(hip_lib):
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()                                # one case's fp64 graph at a time
            cache[name] = _run_ray_case(name)
        return cache[name]
    return get


def test_ray_cases_cover_the_work_split():
    """The matrix reaches what the golden cases do not: tiles_per_ray > 1, tail tiles, tpw >= 8, non-square ray counts."""
    tiles = {k: (c['sc'] + c['sf'] + 31) // 32 for k, c in RAY_CASES.items()}
    tails = {(c['sc'] + c['sf']) % 32 for c in RAY_CASES.values()}
    tpw = {k: min(96, max(1, c['n'] * c['m'] * tiles[k] // 2048)) for k, c in RAY_CASES.items()}
    assert max(tiles.values()) == 4 and {1, 5, 31} <= tails
    assert min(tpw.values()) == 1 and max(tpw.values()) >= 8
    assert any(int(np.sqrt(c['m'])) ** 2 != c['m'] for c in RAY_CASES.values())
    assert {(c['nets'], c.get('sem', False)) for c in RAY_CASES.values()} == {(1, False), (2, False), (2, True)}


@pytest.mark.parametrize('name', list(RAY_CASES))
def test_fused_backward_planes_match_fp64_oracle(ray_case, name):
    r = ray_case(name)
    _check_planes(f'render_bwd_oracle[{name}]', r['gp'], r['ref_p'], r['out']['uv'], B_PLANES)


@pytest.mark.parametrize('name', list(RAY_CASES))
def test_fused_backward_decoder_matches_fp64_oracle(ray_case, name):
    r = ray_case(name)
    _check_decoder(f'render_bwd_oracle[{name}]', r['dec'], r['gd'], r['ref_dec'], B_DEC_EMPTY if name.endswith('_empty') else B_DEC)


@pytest.mark.parametrize('name', list(RAY_CASES))
def test_fused_backward_tape_matches_fp64_oracle(ray_case, name):
    """Colour weight (w[k-1] + w[k]) / 2 and dL/dsigma of every sample, multi-tile S included (the golden-case version of this check,
    test_render_bwd_gpu.py, only reaches one tile per ray)."""
    r = ray_case(name)
    w = r['out']['weights'].detach()
    cw = torch.zeros(w.shape[0], w.shape[1] + 1, dtype=F64, device=w.device)
    cw[:, :-1] += w / 2
    cw[:, 1:] += w / 2
    tape = r['tape']
    assert bool(torch.isfinite(tape[..., :3]).all())
    e_cw, e_ds = _rel(tape[..., 1], cw), _rel(tape[..., 2], r['ref_dsig'])
    record_error(f'render_bwd_oracle[{name}].tape_weight', e_cw)
    record_error(f'render_bwd_oracle[{name}].tape_dsigma', e_ds)
    assert e_cw < B_TAPE and e_ds < B_TAPE, (e_cw, e_ds)


def test_edge_cases_reach_their_regimes(ray_case):
    """The geometry edges are what their names say, measured on the oracle's own evaluation."""
    r = ray_case('seg_24+24_outside_box')
    uv = r['out']['uv']
    outside = (uv.abs() > 1).any(-1).to(F64).mean()
    assert 0.05 < float(outside) < 0.95
    r = ray_case('osg_32+32_empty')
    wsum = r['out']['wsum'].detach()
    assert float((wsum < 1e-4).to(F64).mean()) > 0.15 and float(wsum.max()) > 0.1
    r = ray_case('segsig_32+32_saturated')
    d = r['out']['sigmas'].detach()
    zz = r['tape'][..., 0].to(F64)
    dens = torch.nn.functional.softplus((d[:, :-1] + d[:, 1:]) / 2 - 1) * (zz[:, 1:] - zz[:, :-1])
    sat = (dens[:, :-1] > 17).any(1)                     # alpha rounds to 1 in fp32 before the last interval
    assert float(sat.to(F64).mean()) > 0.3
    assert bool(torch.isfinite(r['gp']).all()) and all(bool(torch.isfinite(x).all()) for x in r['gd'])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the point-query backward (density regularisation: G.sample_mixed, loss.py:681-706)

# 3 x 20 001 points: 1876 tiles of 32 > 1024 (256 blocks x 4 waves) -> the grid-stride loop runs a second round; 20 001 is not a multiple
# of 32, so tiles straddle images and the last tile has a tail.  Coordinates uniform in a box that overhangs the unit box on one side of
# each axis (a share of the points is outside, zero-padded taps) and leaves the other side of every plane untouched.
POINT_CASES = {
    'osg_rgb+sigma': dict(nets=1, sem=False, lr=1.0, rgb=True, n=3, p=20001, hw=(52, 36), cl=False),
    'seg_rgb+sigma_lr': dict(nets=2, sem=False, lr=0.4, rgb=True, n=3, p=20001, hw=(44, 60), cl=True),
    'segsig_sigma_only': dict(nets=2, sem=True, lr=1.0, rgb=False, n=3, p=20001, hw=(36, 28), cl=False),
    'osg_sigma_only': dict(nets=1, sem=False, lr=1.5, rgb=False, n=2, p=777, hw=(20, 30), cl=True),
}


@pytest.mark.parametrize('name', list(POINT_CASES))
def test_point_query_backward_matches_fp64_oracle(hip_lib, name):
    from pix2pix3d_amd.training.volumetric_rendering import renderer as R
    from oracle import render_oracle as RO
    cfg = POINT_CASES[name]
    seed = sorted(POINT_CASES).index(name)
    nets, n, p, (h, w) = cfg['nets'], cfg['n'], cfg['p'], cfg['hw']
    box = 0.9
    opt = dict(box_warp=box)
    dec = _decoder(nets, cfg['sem'], cfg['lr'], 500 + seed)
    planes = _planes(n, h, w, 600 + seed, cfg['cl']).requires_grad_(True)
    g = torch.Generator(device='cuda').manual_seed(700 + seed)
    lo, hi = torch.tensor([-0.6, -0.6, -0.25], device='cuda'), torch.tensor([0.25, 0.3, 0.6], device='cuda')
    xyz = (lo + torch.rand(n, p, 3, device='cuda', generator=g) * (hi - lo)) * box
    g_rgb = torch.randn(n, p, 32 * nets, device='cuda', generator=g) if cfg['rgb'] else None
    g_sig = torch.randn(n, p, 1, device='cuda', generator=g)
    params = list(dec.parameters())
    c0 = R.backward_calls['points']
    rgb, sigma = R._FusedPointsFn.apply(dec, opt, xyz, planes, *params)
    loss = (sigma * g_sig).sum() + ((rgb * g_rgb).sum() if g_rgb is not None else 0.0)
    loss.backward()
    assert R.backward_calls['points'] == c0 + 1
    gp, gd = planes.grad, [q.grad for q in params]

    leaves, d64 = _dec64(dec)
    pl64 = planes.detach().to(F64).contiguous().requires_grad_(True)
    c64, s64 = RO.sample_points_t(pl64, d64, xyz.to(F64), box)
    loss64 = (s64 * g_sig.to(F64)[..., 0]).sum() + ((c64 * g_rgb.to(F64)).sum() if g_rgb is not None else 0.0)
    ref = torch.autograd.grad(loss64, [pl64] + leaves, allow_unused=True)
    uv = RO.plane_coords_t(xyz.to(F64), box)
    outside = float((uv.abs() > 1).any(-1).to(F64).mean())
    assert 0.05 < outside < 0.95

    tag = f'points_bwd_oracle[{name}]'
    _check_planes(tag, gp, ref[0], uv, B_POINTS)
    names = [k for k, _ in dec.named_parameters()]
    if g_rgb is None and nets == 2:                      # only sigma carries a gradient: the colour net is not in the graph
        colour = [i for i, k in enumerate(names) if k.startswith('net.')]
        assert len(colour) == 4 and all(gd[i] is None for i in colour) and all(ref[1 + i] is None for i in colour)
        keep = [i for i in range(len(names)) if i not in colour]
        sub = torch.nn.Module()
        sub.net_semantic = dec.net_semantic
        _check_decoder(tag, sub, [gd[i] for i in keep], [ref[1 + i] for i in keep], B_POINTS)
    else:
        _check_decoder(tag, dec, gd, list(ref[1:]), B_POINTS)
