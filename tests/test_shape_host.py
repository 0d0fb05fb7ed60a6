"""pix2pix3d_amd.shape on the CPU: marching_cubes against a per-cube loop over the table, mesh topology, sigma_grid against the
script's block loop (applications/extract_mesh.py:60-81)."""
import math

import numpy as np
import pytest
import torch

from pix2pix3d_amd import mc_table as M
from pix2pix3d_amd import shape


def brute_marching_cubes(u, threshold):
    """The output contract written out as plain loops: vertices by corner (row-major), then axis; faces by cube, then table order."""
    u = np.asarray(u, dtype=np.float32)
    thr = np.float32(threshold)
    X, Y, Z = u.shape
    vid, verts = {}, []
    for i in range(X):
        for j in range(Y):
            for k in range(Z):
                for a in range(3):
                    n = (i + (a == 0), j + (a == 1), k + (a == 2))
                    if n[0] >= X or n[1] >= Y or n[2] >= Z:
                        continue
                    u0, u1 = u[i, j, k], u[n]
                    if (u0 > thr) == (u1 > thr):
                        continue
                    t = np.float32(np.float32(thr - u0) / np.float32(u1 - u0))
                    p = [np.float32(i), np.float32(j), np.float32(k)]
                    p[a] = np.float32(p[a] + t)
                    vid[(i, j, k, a)] = len(verts)
                    verts.append(p)
    faces = []
    tris = M.triangles()
    for i in range(X - 1):
        for j in range(Y - 1):
            for k in range(Z - 1):
                case = 0
                for c, (dx, dy, dz) in enumerate(M.CORNERS):
                    case |= int(u[i + dx, j + dy, k + dz] > thr) << c
                for t in tris[case]:
                    face = []
                    for e in t:
                        c, a = M.EDGES[e]
                        dx, dy, dz = M.CORNERS[c]
                        face.append(vid[(i + dx, j + dy, k + dz, a)])
                    faces.append(face)
    return np.array(verts, dtype=np.float32).reshape(-1, 3), np.array(faces, dtype=np.int64).reshape(-1, 3)


def _fields():
    g = torch.Generator().manual_seed(3)
    yield 'rand_9x7x11', torch.rand([9, 7, 11], generator=g), 0.5
    yield 'rand_16', torch.randn([16, 16, 16], generator=g), 0.1
    yield 'ties_16', torch.randint(0, 3, [16, 16, 16], generator=g).float(), 1.0     # many corners exactly at the threshold
    yield 'all_inside', torch.ones([5, 6, 7]), 0.0
    yield 'all_outside', torch.zeros([5, 6, 7]), 0.0
    yield 'min_2x2x2', torch.tensor([[[1., 0.], [0., 0.]], [[0., 0.], [0., 1.]]]), 0.5


@pytest.mark.parametrize('name,u,thr', list(_fields()), ids=[f[0] for f in _fields()])
def test_cpu_path_equals_the_per_cube_loop(name, u, thr):
    v, f = shape.marching_cubes(u, thr)
    bv, bf = brute_marching_cubes(u.numpy(), thr)
    assert v.dtype == torch.float32 and f.dtype == torch.int64 and v.shape[1] == 3 and f.shape[1] == 3
    assert np.array_equal(f.numpy(), bf)
    assert v.numpy().tobytes() == bv.tobytes()
    if name.startswith('all_'):
        assert v.shape == (0, 3) and f.shape == (0, 3)


def check_closed_oriented(faces, n_vertices):
    """Every undirected edge is used by exactly two faces, once in each direction; every vertex is used.  Returns V - E + F."""
    f = np.asarray(faces)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    assert (d[:, 0] != d[:, 1]).all()
    key = d[:, 0].astype(np.int64) * n_vertices + d[:, 1]
    rkey = d[:, 1].astype(np.int64) * n_vertices + d[:, 0]
    assert len(np.unique(key)) == len(key), 'a directed edge is used twice'
    assert np.isin(rkey, key).all(), 'an edge is used in one direction only'
    assert len(np.unique(f)) == n_vertices
    return n_vertices - len(key) // 2 + len(f)


def signed_volume(v, f):
    v = np.asarray(v, dtype=np.float64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)


def sphere(n, r, centre=None):
    c = torch.tensor(centre if centre is not None else [(n - 1) / 2 + 0.17, (n - 1) / 2 - 0.23, (n - 1) / 2 + 0.05], dtype=torch.float64)
    g = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64)] * 3, indexing='ij'), -1)
    return (r - (g - c).norm(dim=-1)).float()


def torus(shape_, big, small):
    c = torch.tensor([(s - 1) / 2 + 0.1 for s in shape_], dtype=torch.float64)
    g = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in shape_], indexing='ij'), -1) - c
    q = torch.sqrt(g[..., 0] ** 2 + g[..., 1] ** 2) - big
    return (small - torch.sqrt(q ** 2 + g[..., 2] ** 2)).float()


def test_sphere_is_a_closed_sphere_of_the_right_volume():
    r = 20.0
    v, f = shape.marching_cubes(sphere(48, r), 0.0)
    assert check_closed_oriented(f.numpy(), len(v)) == 2
    vol = signed_volume(v.numpy(), f.numpy())
    exact = 4.0 / 3.0 * math.pi * r ** 3
    assert vol > 0 and abs(vol - exact) / exact < 0.01, (vol, exact)


def test_torus_has_euler_characteristic_zero():
    v, f = shape.marching_cubes(torus([40, 40, 20], 12.0, 5.0), 0.0)
    assert check_closed_oriented(f.numpy(), len(v)) == 0
    assert signed_volume(v.numpy(), f.numpy()) > 0


@pytest.mark.parametrize('seed', range(3))
def test_noise_with_outside_border_is_closed(seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand([14, 12, 13], generator=g)
    u[0], u[-1], u[:, 0], u[:, -1], u[:, :, 0], u[:, :, -1] = 0, 0, 0, 0, 0, 0
    v, f = shape.marching_cubes(u, 0.5)
    assert len(f) > 100
    check_closed_oriented(f.numpy(), len(v))
    assert signed_volume(v.numpy(), f.numpy()) > 0


def test_marching_cubes_rejects_flat_fields():
    with pytest.raises(ValueError):
        shape.marching_cubes(torch.zeros([1, 4, 4]), 0.0)


def test_entry_points_reject_what_their_index_types_cannot_hold():
    """Argument checks of csrc/shape.hip: error codes and messages, returned before any launch (no GPU needed)."""
    import ctypes
    from pix2pix3d_amd import _lib
    from pix2pix3d_amd.training.volumetric_rendering import renderer as rmod
    h = _lib.lib()
    dummy = ctypes.c_void_p(16)
    assert h.p3d_marching_cubes_classify(dummy, 1, 8, 8, 0.0, dummy, dummy, dummy, None) == -2
    assert b'>= 2' in h.p3d_last_error()
    assert h.p3d_marching_cubes_blocks(2, 2, 2) == 1 and h.p3d_marching_cubes_blocks(512, 512, 512) == 512 ** 3 // 256
    assert h.p3d_marching_cubes_emit(dummy, 8, 8, 8, 0.0, dummy, dummy, dummy, dummy, 2 ** 31, 10, dummy, dummy, dummy, None) == -1
    assert b'32-bit vertex ids' in h.p3d_last_error()
    d = rmod._RenderDesc(86, 1, 256, 256, 2, 0, 0, 0, 0, 0, 0.0, 0.0, 1.0, 0, 0, 0, 0, 0)      # 86 x 3 x 256^2 x 32 floats: > 2^31 bytes
    assert h.p3d_sample_lattice(dummy, dummy, ctypes.byref(d), dummy, dummy, dummy, 4, 4, 4, dummy, None) == -1
    assert b'32-bit buffer addressing' in h.p3d_last_error()
    d.n_img = 1
    assert h.p3d_sample_lattice(dummy, dummy, ctypes.byref(d), dummy, dummy, dummy, 2048, 2048, 1024, dummy, None) == -1
    assert b'32-bit in-image index' in h.p3d_last_error()


def _plane_desc_callers():
    """name -> (call(descriptor or None, missing=False), honours shared planes, one grid row per set): every entry point that reads the tri-plane
    features through a p3d_render_desc, with dummy non-null pointers and otherwise valid arguments.  ``missing`` nulls one required output."""
    import ctypes
    from pix2pix3d_amd import _lib
    h = _lib.lib()
    p = ctypes.c_void_p(16)
    return {
        'p3d_sample_points': (lambda d, missing=False: h.p3d_sample_points(p, p, p, d, 64, p, p, None), False, False),      # csrc/render.hip: the yardstick
        'p3d_sample_lattice': (lambda d, missing=False: h.p3d_sample_lattice(p, p, d, p, p, p, 4, 4, 4, p, None), False, True),
        'p3d_surface_cast': (lambda d, missing=False: h.p3d_surface_cast(p, p, d, p, p, 0.1, 0.1, 8, 2, 10.0, 0.01, 0.5, 0, None if missing else p, p, p, p,
                                                                         None), True, True),
        'p3d_surface_occlusion': (lambda d, missing=False: h.p3d_surface_occlusion(p, p, d, p, p, p, p, 3, 0.1, 4, 10.0, 0.5, 0, None if missing else p, p,
                                                                                   None), True, True),
        'p3d_render_backward': (lambda d, missing=False: h.p3d_render_backward(p, p, p, p, p, p, p, None, None, d, p, p, p, p, p, p, None), False, False),
        'p3d_sample_points_backward': (lambda d, missing=False: h.p3d_sample_points_backward(p, p, p, p, d, 64, p, p, p, p, None), False, False),
    }


def _plane_desc(**over):
    from pix2pix3d_amd.training.volumetric_rendering import renderer as rmod
    fields = dict(n_img=1, rays_per_img=64, plane_h=16, plane_w=16, n_nets=2, semantic_sigmoid=0, depth_resolution=8, depth_resolution_importance=8,
                  disparity_space_sampling=0, white_back=0, ray_start=0.1, ray_end=1.0, box_warp=1.0, image_stride=0, plane_stride=0, pixel_stride=0,
                  raster_order=0, mlp_bf16x3=0)
    fields.update(over)
    return rmod._RenderDesc(**fields)


def _strided(pixel_stride):      # the [N][H][W][C] view: the three planes interleaved in a pixel's channels
    return dict(pixel_stride=pixel_stride, plane_stride=32, image_stride=pixel_stride * 16 * 16)


# (row, descriptor fields or None for a null descriptor, return code, what the message says)
_BAD_PLANE_DESCS = [
    ('null', None, -2, b'null descriptor'),
    ('n_nets_3', dict(n_nets=3), -2, b'n_nets must be 1 or 2'),
    ('plane_h_0', dict(plane_h=0), -2, b'bad plane size'),
    ('box_warp_0', dict(box_warp=0.0), -2, b'box_warp must be non-zero'),
    ('over_2GiB', dict(n_img=86, plane_h=256, plane_w=256), -1, b'32-bit buffer addressing'),      # 86 x 3 x 256^2 x 32 floats: > 2^31 bytes
    ('pixel_stride_16384', _strided(16384), -1, b'32-bit buffer addressing'),                      # 65536 bytes: past the 24-bit multiply's 16-bit factor
    ('pixel_stride_98', _strided(98), -2, b'16-byte aligned'),
]


@pytest.mark.parametrize('entry', ['p3d_sample_lattice', 'p3d_surface_cast', 'p3d_surface_occlusion', 'p3d_render_backward', 'p3d_sample_points_backward'])
def test_every_plane_reader_rejects_what_the_point_kernel_rejects(entry):
    """csrc/render_host.h's check_plane_desc behind every entry point that reads the planes: the codes of p3d_sample_points (csrc/render.hip, which keeps
    its own copy of the checks) and, after the ``who:`` prefix, its messages — all returned before any launch (no GPU needed)."""
    import ctypes
    from pix2pix3d_amd import _lib
    h = _lib.lib()
    callers = _plane_desc_callers()
    call, shared, set_rows = callers[entry]
    yardstick = callers['p3d_sample_points'][0]

    def message():
        return h.p3d_last_error().split(b': ', 1)[1]

    for row, fields, code, says in _BAD_PLANE_DESCS:
        d = None if fields is None else ctypes.byref(_plane_desc(**fields))
        assert yardstick(d) == code, row
        want = message()
        assert says in want, (row, want)
        assert call(d) == code, row
        assert message() == want, row
    if set_rows:
        assert call(ctypes.byref(_plane_desc(n_img=65536))) == -2
        assert b'n_img must be in [0, 65535]' in message()
    over = dict(n_img=86, plane_h=256, plane_w=256, raster_order=2)      # P3D_RENDER_SHARED_PLANES: one 256^2 set under 86 ray sets
    if shared:      # the span is the one set's: the descriptor passes, the next bad argument is reported
        assert call(ctypes.byref(_plane_desc(**over)), missing=True) == -2
        assert message() == b'null pointer'
    else:           # the bit is ignored: 86 sets
        assert call(ctypes.byref(_plane_desc(**over))) == -1
        assert b'32-bit buffer addressing' in message()


def script_sigma_field(G, ws, resolution, block_resolution=64):
    """get_sigma_field_np (extract_mesh.py:60-81) restated for one image."""
    bound = G.rendering_kwargs['box_warp'] * 0.5
    X = torch.linspace(-bound, bound, resolution).split(block_resolution)
    out = np.zeros([resolution] * 3, dtype=np.float32)
    for xi, xs in enumerate(X):
        for yi, ys in enumerate(X):
            for zi, zs in enumerate(X):
                xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing='ij')
                pts = torch.stack([xx, yy, zz], dim=-1).unsqueeze(0).to(ws.device)
                sig = G.sample_mixed(pts.reshape(1, -1, 3), None, ws=ws, noise_mode='const')['sigma']
                out[xi * block_resolution:xi * block_resolution + len(xs), yi * block_resolution:yi * block_resolution + len(ys),
                    zi * block_resolution:zi * block_resolution + len(zs)] = sig.reshape(len(xs), len(ys), len(zs)).detach().cpu().numpy()
    return out


@pytest.mark.parametrize('name', ['seg2cat', 'edge2car'])
def test_sigma_grid_cpu_equals_the_script_loop(name):
    from model_cases import build_generator
    G = build_generator(name)
    ws = torch.randn([1, G.backbone.num_ws, 512], generator=torch.Generator().manual_seed(5))
    u = shape.sigma_grid(G, ws, resolution=16)
    assert u.shape == (1, 16, 16, 16) and u.dtype == torch.float32
    with torch.no_grad():
        ref = script_sigma_field(G, ws, 16)
    assert np.array_equal(u[0].numpy(), ref)
    assert float(u.std()) > 0
