"""The forward ray-marcher after its per-sample vector work was cut (csrc/render_device.h): softplus with one wave-uniform threshold branch,
the sigmoid's scaling and clamping moved out of the decode loop, one fma per channel in the composite, the 1/3 of the plane mean in layer 1's
weights, and the label net's squashing as a template parameter.

Bounds are the ones tests/test_render_gpu.py holds against the numpy oracle: features and wsum rel_err < 2e-4, depth < 5e-5."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import render_oracle as R
from render_cases import CASES, load_case, make_decoder

pytestmark = pytest.mark.gpu

FORMS = ['bf16x3', 'l1x6', 'exact']          # p3d_render_desc.mlp_bf16x3 = 1, 2, 0: the three decoder forms of the one-plane-set forward kernel


def _rmod():
    from pix2pix3d_amd.training.volumetric_rendering import renderer
    return renderer


def _launch(form, planes, dec, o, d, opts, uc, uf, t0=None, t1=None):
    """One fused launch with the decoder in the given form -> (feat [N,M,C], depth [N,M], wsum [N,M]), device tensors."""
    rmod = _rmod()
    from pix2pix3d_amd.torch_utils.ops import modconv
    prev = (rmod.mlp_bf16x3, rmod.mlp_l1x6, modconv.f32_x6)
    try:
        rmod.mlp_bf16x3, rmod.mlp_l1x6, modconv.f32_x6 = form == 'bf16x3', form == 'l1x6', form == 'l1x6'
        out = rmod.fused_render(planes, dec, o, d, opts, uc, uf, t0, t1, exact_fp32=form != 'bf16x3')
    finally:
        rmod.mlp_bf16x3, rmod.mlp_l1x6, modconv.f32_x6 = prev
    assert out is not None
    feat, depth, wsum = out
    return feat, depth[..., 0], wsum[..., 0]


def _within_oracle_bounds(got, ref, what):
    feat, depth, wsum = (t.cpu().numpy() if torch.is_tensor(t) else t for t in got)
    fo, do, wo = ref
    e = rel_err(feat, fo), float(np.abs(depth - do).max()), rel_err(wsum, wo)
    print(what, 'feat rel_err %.3g  depth abs %.3g  wsum rel_err %.3g' % e)
    assert e[0] < 2e-4 and e[1] < 5e-5 and e[2] < 2e-4, (what, e)


# ---- 1. the softplus paths give the same bits: a ray's result does not depend on its wave-mates ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hot_corner_scene():
    """One image of 8 x 8-texel planes, 64 rays (two waves by linear assignment), 8 + 8 samples.  Texels [6:8, 6:8] of every plane hold features of
    about 1e3, everything else is benign; the rays run along +z through 2 p in [-0.8, 0.25]^3, far from those texels.  The `hot` variant moves ray 5
    to x = y = 0.42 (2 p = 0.84: taps 6 and 7 of the (x, y) plane), where hidden pre-activations pass the softplus threshold and the exp2's range."""
    g, opts, dec_arrays = load_case('seg')
    opts = dict(opts, depth_resolution=8, depth_resolution_importance=8, ray_start=0.1, ray_end=0.5, box_warp=1, disparity_space_sampling=False, white_back=False)
    rng = np.random.RandomState(7)                # (a seed at which the hot texels are dense: ray 5 composites label logits of about 1e3, w_sum = 1)
    planes = (0.5 * rng.randn(1, 3, 32, 8, 8)).astype(np.float32)
    planes[:, :, :, 6:8, 6:8] = (1e3 * rng.randn(1, 3, 32, 2, 2)).astype(np.float32)
    o = np.zeros([1, 64, 3], np.float32)
    o[0, :, 0], o[0, :, 1], o[0, :, 2] = rng.uniform(-0.4, 0.0, 64), rng.uniform(-0.4, 0.0, 64), -0.45
    d = np.tile(np.array([[[0.0, 0.0, 1.0]]], np.float32), [1, 64, 1])
    o_hot = o.copy()
    o_hot[0, 5, :2] = 0.42
    uc = rng.rand(1, 64, 8).astype(np.float32)
    uf = rng.rand(64, 8).astype(np.float32)
    ref_hot = R.render(planes, dec_arrays, o_hot, d, opts, uc, uf)
    # the scene does what it is for: hidden pre-activations of ray 5 above the threshold (20) and above exp's range (88.7), none such on the benign rays
    z = R.sample_stratified(uc, opts['ray_start'], opts['ray_end'])

    def pre(origins):
        pts = (origins[:, :, None, :] + z[..., None] * d[:, :, None, :]).reshape(1, -1, 3)
        x = R.sample_from_planes(planes, pts, opts['box_warp']).mean(1)
        return np.concatenate([R._fc(x, dec_arrays['w1' + s], dec_arrays['b1' + s], dec_arrays['lr_mul']) for s in ('', 's')], -1).reshape(64, 8, -1)
    x_hot, x_cold = pre(o_hot), pre(o)
    assert (x_hot[5] > 88.7).any() and ((x_hot[5] > 20) & (x_hot[5] < 88.7)).any() and x_cold.max() < 20 and np.delete(x_hot, 5, 0).max() < 20
    assert ref_hot[2][0, 5] > 0.99 and np.abs(ref_hot[0][0, 5]).max() > 100
    return g, opts, planes, o, o_hot, d, uc, uf, ref_hot


@pytest.mark.parametrize('form', FORMS)
def test_wave_mates_do_not_matter(hip_lib, form):
    g, opts, planes, o, o_hot, d, uc, uf, ref_hot = _hot_corner_scene()
    dec = make_decoder(g, 'cuda')
    t = lambda a: torch.tensor(a, device='cuda')
    cold = _launch(form, t(planes), dec, t(o), t(d), opts, t(uc), t(uf))
    hot = _launch(form, t(planes), dec, t(o_hot), t(d), opts, t(uc), t(uf))
    others = torch.arange(64, device='cuda') != 5
    for a, b, what in zip(cold, hot, ('feat', 'depth', 'wsum')):
        assert torch.equal(a[:, others], b[:, others]), (form, what)          # the fast and the slow softplus path: the same bits
        assert not torch.equal(a[:, 5], b[:, 5]) or what == 'depth', (form, what)
    assert all(torch.isfinite(v[:, 5]).all() for v in hot)
    _within_oracle_bounds([v[:, 5:6] for v in hot], [v[:, 5:6] for v in ref_hot], f'hot ray, {form}:')
    _within_oracle_bounds(hot, ref_hot, f'all rays, {form}:')


# ---- 2. every template variant against the oracle at the recorded cases ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case_reference(name, flip):
    """The recorded case, or (flip) the same with the label net's squashing and the white background toggled — and the oracle's render of it."""
    g, opts, dec_arrays = load_case(name)
    if flip:
        opts = dict(opts, white_back=not opts.get('white_back', False))
        dec_arrays = dict(dec_arrays, semantic_sigmoid=not dec_arrays['semantic_sigmoid'])
    return g, opts, dec_arrays


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('name', CASES)
def test_variants_match_the_oracle(hip_lib, name, form, flip):
    """n_nets 1 ('osg') and 2; linear ('seg', 'car'), disparity ('osg') and per-ray 'auto' limits; semantic_sigmoid and white_back as recorded and flipped."""
    rmod = _rmod()
    g, opts, dec_arrays = _case_reference(name, flip)
    dec = make_decoder(g, 'cuda')
    if int(g['nets']) == 2:
        dec.semantic_sigmoid = dec_arrays['semantic_sigmoid']
    t = lambda a: torch.tensor(a, device='cuda')
    o, d = t(g['ray_o']), t(g['ray_d'])
    t0 = t1 = None
    kw = {}
    if opts['ray_start'] == 'auto':
        t0, t1 = rmod.ImportanceRenderer()._ray_limits(o, d, opts)
        kw = dict(t_start=t0.cpu().numpy(), t_end=t1.cpu().numpy())
    ref = R.render(g['planes'], dec_arrays, g['ray_o'], g['ray_d'], opts, g['u_coarse'], g['u_fine'], **kw)
    got = _launch(form, t(g['planes']), dec, o, d, opts, t(g['u_coarse']), t(g['u_fine']), t0, t1)
    _within_oracle_bounds(got, ref, f'{name} {form} flip={flip}:')


# ---- 3. the affine part of the clamped sigmoid, applied once per ray --------------------------------------------------------------------------------
@pytest.mark.parametrize('form', FORMS)
def test_affine_fold_edge_cases(hip_lib, form):
    """37 rays (tail lanes), 8 + 7 samples (an odd total).  Empty space: acc = 0 and w_sum = 0, so 1.002 acc - 0.001 w_sum must be exactly 0;
    a saturated first interval: w_sum = 1 and the colours stay inside sigmoid_clamped's range."""
    g, opts, dec_arrays = load_case('seg')
    opts = dict(opts, depth_resolution=8, depth_resolution_importance=7)
    dec = make_decoder(g, 'cuda')
    n, m = 1, 37
    rng = np.random.RandomState(3)
    planes = rng.randn(n, 3, 32, 8, 8).astype(np.float32)
    o = np.concatenate([g['ray_o'][:1], g['ray_o'][:1, :1]], 1)
    d = np.concatenate([g['ray_d'][:1], g['ray_d'][1:2, :1]], 1)
    uc, uf = rng.rand(n, m, 8).astype(np.float32), rng.rand(n * m, 7).astype(np.float32)
    t = lambda a: torch.tensor(a, device='cuda')
    args = (t(planes), dec, t(o), t(d), opts, t(uc), t(uf))
    _within_oracle_bounds(_launch(form, *args), R.render(planes, dec_arrays, o, d, opts, uc, uf), f'37 rays, 8 + 7, {form}:')
    with torch.no_grad():
        dec.net_semantic[2].bias[0] = -1e4
    feat, depth, wsum = _launch(form, *args)
    print(form, 'empty space: max |feat + 1| %.3g  max wsum %.3g' % (float((feat + 1).abs().max()), float(wsum.max())))
    assert float((feat + 1).abs().max()) <= 1e-5 and float(wsum.max()) < 1e-6 and torch.isfinite(depth).all()
    with torch.no_grad():
        dec.net_semantic[2].bias[0] = 50.0
    feat, depth, wsum = _launch(form, *args)
    print(form, 'saturated: max |wsum - 1| %.3g  colour range [%.6f, %.6f]' % (float((wsum - 1).abs().max()), float(feat[..., :32].min()), float(feat[..., :32].max())))
    assert float((wsum - 1).abs().max()) <= 1e-5
    assert float(feat[..., :32].min()) >= -1.0021 and float(feat[..., :32].max()) <= 1.0021
    dec_sat = dict(dec_arrays, b2s=dec_arrays['b2s'].copy())
    dec_sat['b2s'][0] = 50.0
    _within_oracle_bounds((feat, depth, wsum), R.render(planes, dec_sat, o, d, opts, uc, uf), f'saturated, {form}:')


# ---- 4. first / last sample of the re-associated composite -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', FORMS)
def test_shortest_ray_first_and_last_fold(hip_lib, form):
    """The fewest samples the fused kernel takes: 4 + 1 (five samples, four intervals; p3d_render_forward reports depth_resolution < 4 as unsupported — the
    importance sampler needs depth_resolution - 3 >= 1 pdf entries — so a 2 + 1 ray cannot be launched).  Each sample is folded with the half weights of the
    intervals on both its sides, the first and the last with one: a dropped last fold or a double-counted first one moves the colours by that interval's
    share, which the scene keeps large (checked on the oracle's weights)."""
    rmod = _rmod()
    g, opts, dec_arrays = load_case('seg')
    dec = make_decoder(g, 'cuda')
    t = lambda a: torch.tensor(a, device='cuda')
    rng = np.random.RandomState(11)
    n, m = g['ray_o'].shape[:2]
    short = dict(opts, depth_resolution=2, depth_resolution_importance=1)
    assert rmod.fused_render(t(g['planes']), dec, t(g['ray_o']), t(g['ray_d']), short, t(rng.rand(n, m, 2).astype(np.float32)), t(rng.rand(n * m, 1).astype(np.float32))) is None
    opts = dict(opts, depth_resolution=4, depth_resolution_importance=1)
    uc, uf = rng.rand(n, m, 4).astype(np.float32), rng.rand(n * m, 1).astype(np.float32)
    ref = R.render(g['planes'], dec_arrays, g['ray_o'], g['ray_d'], opts, uc, uf, details=True)
    det = ref[3]
    _, _, w = R.ray_march(det['colors'], det['sigmas'], det['z_all'])
    share = w / np.maximum(w.sum(1, keepdims=True), 1e-30)
    print('median share of the first / last interval: %.3g / %.3g' % (np.median(share[:, 0]), np.median(share[:, -1])))
    assert np.median(share[:, 0]) > 0.02 and np.median(share[:, -1]) > 0.02           # both ends carry weight: far above the 2e-4 bound
    got = _launch(form, t(g['planes']), dec, t(g['ray_o']), t(g['ray_d']), opts, t(uc), t(uf))
    _within_oracle_bounds(got, ref[:3], f'4 + 1 samples, {form}:')
