"""pix2pix3d_amd.shape on the device: the density lattice kernel against the point kernel (bit for bit) and the tensor-op restatement,
marching cubes against the CPU path, extract_geometry against applications/extract_mesh.py's loop."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from model_cases import build_generator
from pix2pix3d_amd import _lib, shape
from pix2pix3d_amd.training.volumetric_rendering import renderer as rmod
from test_shape_host import brute_marching_cubes, check_closed_oriented, script_sigma_field, signed_volume, sphere

pytestmark = pytest.mark.gpu


def _decoder(nets, seed):
    from pix2pix3d_amd.training.triplane import OSGDecoder
    from pix2pix3d_amd.training.triplane_cond import OSGDecoder_semantic_lateSeparate
    torch.manual_seed(seed)
    if nets == 1:
        dec = OSGDecoder(32, {'decoder_lr_mul': 1.0, 'decoder_output_dim': 32})
    else:
        dec = OSGDecoder_semantic_lateSeparate(32, {'decoder_lr_mul': 1.0, 'decoder_output_dim': 32, 'sigmoid': False, 'semantic_channels': 6})
    return dec.eval().requires_grad_(False)


def _lattice_points(axis, n):
    xx, yy, zz = torch.meshgrid(axis, axis, axis, indexing='ij')
    return torch.stack([xx, yy, zz], -1).reshape(1, -1, 3).expand(n, -1, -1).contiguous()


@pytest.mark.parametrize('nets', [1, 2])
@pytest.mark.parametrize('res', [37, 48])
def test_lattice_equals_point_kernel_and_tensor_ops(hip_lib, nets, res):
    g = torch.Generator().manual_seed(10 * nets + res)
    planes = torch.randn([2, 3, 32, 64, 64], generator=g) * 2
    dec = _decoder(nets, seed=nets)
    opt = {'box_warp': 1.0}
    axis = torch.linspace(-0.55, 0.55, res)                        # a little beyond the box: zero-padded taps at the border
    pts = _lattice_points(axis, 2)
    n0 = _lib.launch_count('render')
    with torch.no_grad():
        lat = rmod.fused_sample_lattice(planes.cuda(), dec.cuda(), axis, axis, axis, opt)
        pt = rmod.fused_sample_points(planes.cuda(), dec.cuda(), pts.cuda(), opt)[1]
        ref = rmod.ImportanceRenderer()._points_tensor_ops(planes, dec.cpu(), pts, None, opt)['sigma']
    torch.cuda.synchronize()
    assert _lib.launch_count('render') >= n0 + 2
    assert lat.shape == (2, res, res, res)
    assert torch.equal(lat.cpu(), pt.reshape(2, res, res, res).cpu())
    assert rel_err(lat.cpu().numpy(), ref.reshape(2, res, res, res).numpy()) < 1e-3


@pytest.mark.parametrize('name', ['seg2cat', 'edge2car'])
@pytest.mark.parametrize('res', [37, 48])
def test_sigma_grid_equals_sample_mixed(hip_lib, name, res):
    G = build_generator(name, 'cuda')
    ws = torch.randn([2, G.backbone.num_ws, 512], generator=torch.Generator().manual_seed(res)).cuda()
    bound = G.rendering_kwargs['box_warp'] * 0.5
    prev, rmod.fused_policy = rmod.fused_policy, 'require'
    try:
        n0 = _lib.launch_count('render')
        u = shape.sigma_grid(G, ws, resolution=res)
        torch.cuda.synchronize()
        assert _lib.launch_count('render') > n0
        with torch.no_grad():
            pts = _lattice_points(torch.linspace(-bound, bound, res), 2).cuda()
            sm = G.sample_mixed(pts, None, ws, noise_mode='const')['sigma']
    finally:
        rmod.fused_policy = prev
    assert u.shape == (2, res, res, res) and u.is_cuda
    assert torch.equal(u, sm.reshape(2, res, res, res))
    assert float(u.std()) > 0


def test_lattice_beyond_one_point_launch(hip_lib):
    """384^3 = 56.6 M points: more than p3d_sample_points takes in one call (INT32_MAX / 64); 100 k entries against the point kernel."""
    G = build_generator('seg2cat', 'cuda')
    ws = torch.randn([1, G.backbone.num_ws, 512], generator=torch.Generator().manual_seed(1)).cuda()
    res = 384
    u = shape.sigma_grid(G, ws, resolution=res)
    axis = torch.linspace(-G.rendering_kwargs['box_warp'] * 0.5, G.rendering_kwargs['box_warp'] * 0.5, res)
    idx = torch.randint(0, res, [100_000, 3], generator=torch.Generator().manual_seed(2))
    pts = axis[idx].reshape(1, -1, 3).cuda()
    with torch.no_grad():
        planes = shape._planes(G, ws, noise_mode='const')
        ref = rmod.fused_sample_points(planes, G.decoder, pts, G.rendering_kwargs)[1].reshape(-1)
    got = u[0][idx[:, 0].cuda(), idx[:, 1].cuda(), idx[:, 2].cuda()]
    assert torch.equal(got, ref)
    assert torch.isfinite(u).all()


def test_sigma_grid_fallback_follows_policy(hip_lib):
    G = build_generator('edge2car', 'cuda')
    ws = torch.zeros([1, G.backbone.num_ws, 512], device='cuda')
    rk = G.rendering_kwargs
    prev, rmod.fused_policy = rmod.fused_policy, 'require'
    try:
        G.rendering_kwargs = dict(rk, density_noise=1.0)
        with pytest.raises(RuntimeError, match='lattice kernel required'):
            shape.sigma_grid(G, ws, resolution=8)
    finally:
        G.rendering_kwargs = rk
        rmod.fused_policy = prev


def _mc_fields():
    g = torch.Generator().manual_seed(4)
    yield 'sphere_64', sphere(64, 25.0), 0.0
    yield 'rand_40x33x29', torch.randn([40, 33, 29], generator=g), 0.2
    yield 'ties', torch.randint(0, 3, [23, 31, 17], generator=g).float(), 1.0
    yield 'empty', torch.zeros([9, 10, 11]), 0.5
    yield 'full', torch.ones([9, 10, 11]), 0.5


@pytest.mark.parametrize('name,u,thr', list(_mc_fields()), ids=[f[0] for f in _mc_fields()])
def test_marching_cubes_device_equals_cpu(hip_lib, name, u, thr):
    n0 = _lib.launch_count('aux')
    v, f = shape.marching_cubes(u.cuda(), thr)
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') > n0
    cv, cf = shape.marching_cubes(u, thr)
    assert v.is_cuda and f.is_cuda and v.dtype == torch.float32 and f.dtype == torch.int64
    assert torch.equal(f.cpu(), cf)
    assert v.cpu().numpy().tobytes() == cv.numpy().tobytes()
    if name in ('empty', 'full'):
        assert v.shape == (0, 3) and f.shape == (0, 3)
    if name == 'rand_40x33x29':                                      # and the contract written out as loops
        bv, bf = brute_marching_cubes(u.numpy(), thr)
        assert np.array_equal(f.cpu().numpy(), bf) and v.cpu().numpy().tobytes() == bv.tobytes()


def test_marching_cubes_on_a_lattice(hip_lib):
    G = build_generator('seg2cat', 'cuda')
    ws = torch.randn([1, G.backbone.num_ws, 512], generator=torch.Generator().manual_seed(3)).cuda()
    u = shape.sigma_grid(G, ws, resolution=96)[0]
    thr = float(u.median())
    v, f = shape.marching_cubes(u, thr)
    cv, cf = shape.marching_cubes(u.cpu(), thr)
    assert len(cf) > 1000
    assert torch.equal(f.cpu(), cf) and v.cpu().numpy().tobytes() == cv.numpy().tobytes()


def test_marching_cubes_512_sphere(hip_lib):
    n, r = 512, 200.0
    a = torch.arange(n, dtype=torch.float32, device='cuda')
    c = (n - 1) / 2 + 0.3
    u = r - torch.sqrt((a.view(-1, 1, 1) - c) ** 2 + (a.view(1, -1, 1) - c) ** 2 + (a.view(1, 1, -1) - c) ** 2)
    v1, f1 = shape.marching_cubes(u, 0.0)
    v2, f2 = shape.marching_cubes(u, 0.0)
    assert torch.equal(v1, v2) and torch.equal(f1, f2)
    v, f = v1.cpu().numpy(), f1.cpu().numpy()
    assert check_closed_oriented(f, len(v)) == 2
    vol, exact = signed_volume(v, f), 4.0 / 3.0 * np.pi * r ** 3
    assert vol > 0 and abs(vol - exact) / exact < 0.01


def test_extract_geometry_equals_the_script(hip_lib):
    G = build_generator('seg2cat', 'cuda')
    ws = torch.randn([1, G.backbone.num_ws, 512], generator=torch.Generator().manual_seed(6)).cuda()
    res = 128
    thr = float(shape.sigma_grid(G, ws, resolution=res).median())
    prev, rmod.fused_policy = rmod.fused_policy, 'require'
    try:
        v, f = shape.extract_geometry(G, ws, resolution=res, threshold=thr)
        with torch.no_grad():
            u = script_sigma_field(G, ws, res)                           # the script's device blocks, copied to the host
    finally:
        rmod.fused_policy = prev
    rv, rf = shape.marching_cubes(torch.from_numpy(u), thr)
    bound = G.rendering_kwargs['box_warp'] * 0.5
    rv = (rv.numpy().astype(np.float64) / (res - 1.0) * (bound - -bound) + -bound).astype('float32')
    assert len(rf) > 1000
    assert torch.equal(f.cpu(), rf)
    assert float(np.abs(v.cpu().numpy() - rv).max()) <= 1e-6
