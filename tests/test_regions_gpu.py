"""pix2pix3d_amd.regions on the device: the bytes of p3d_label_components / p3d_label_nearest / p3d_label_warp against the CPU formulation (integer equality, the
kernels' own launch counter moving), and one session at seg2cat bench size that scales one label, removes another and renders."""
import numpy as np
import pytest
import torch

from views_cases import to_device_same_layout
from edit_cases import random_mask, Counters
from regions_cases import spiral, checkerboard
from test_edit_gpu import bench_session, _bytes_apart          # noqa: F401  (the fixture and the helper of the edit tests, reused as they are)

pytestmark = pytest.mark.gpu


def _view_in_canvas(mask, shift):
    """``mask`` as a device view with row pitch W + 6 and a pointer ``shift`` bytes off a 4-byte boundary pattern, inside a larger canvas."""
    h, w = mask.shape
    store = torch.full([(h + 2) * (w + 6) + 8], 77, dtype=torch.uint8)
    view = store[shift:shift + (h + 2) * (w + 6)].view(h + 2, w + 6)[1:1 + h, 2:2 + w]
    view.copy_(mask)
    dev = to_device_same_layout(view)
    assert dev.stride(0) == w + 6 and torch.equal(dev.cpu(), mask)
    return dev


def _ran(n0, launches):
    from pix2pix3d_amd import regions
    torch.cuda.synchronize()
    assert regions.launch_count() == n0 + launches, (regions.launch_count() - n0, launches)


# ---- 1. components ----------------------------------------------------------------------------------------------------------------
def _component_cases():
    return {'spiral 64': spiral(64), 'checkerboard 67x131': checkerboard(67, 131), '1x1': torch.full([1, 1], 3, dtype=torch.uint8),
            '1x300': random_mask(1, 1, 300, 4, seed=5)[0], '300x1': random_mask(1, 300, 1, 4, seed=6)[0], 'blobs 512': random_mask(1, 512, 512, 6, seed=7)[0]}


@pytest.fixture(scope='module')
def component_refs():
    """{(name, connectivity): (mask, CPU ids)}: computed once, never modified."""
    from pix2pix3d_amd import regions
    return {(name, c): (mask, regions.components(mask, c)) for name, mask in _component_cases().items() for c in (4, 8)}


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('name', sorted(_component_cases()))
def test_components_equal_the_cpu_formulation(hip_lib, component_refs, name, connectivity):
    """The spiral is one chain of ~2000 pixels across every 64-pixel boundary: an incomplete flatten or a lost hook shows there; the checkerboard has the most
    components (4) or two interleaved ones joined by diagonals only (8), at an odd width."""
    from pix2pix3d_amd import regions
    mask, want = component_refs[name, connectivity]
    n0 = regions.launch_count()
    ids = regions.components(mask.cuda(), connectivity)
    _ran(n0, 3)
    assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.is_cuda
    bad = int((ids.cpu() != want).sum())
    print(name, connectivity, 'components', len(want.unique()), 'differing ids', bad)
    assert bad == 0


@pytest.mark.parametrize('connectivity', [4, 8])
def test_components_of_a_pitched_misaligned_view(hip_lib, connectivity):
    from pix2pix3d_amd import regions
    mask = random_mask(1, 67, 131, 19, seed=8)[0]
    want = regions.components(mask, connectivity)
    for shift in (1, 2, 3):
        n0 = regions.launch_count()
        ids = regions.components(_view_in_canvas(mask, shift), connectivity)
        _ran(n0, 3)
        assert torch.equal(ids.cpu(), want), (connectivity, shift)


# ---- 2. nearest ------------------------------------------------------------------------------------------------------------------
def _nearest_equal(mask, sites, radius, dev=None):
    from pix2pix3d_amd import regions
    want = regions.nearest(mask, sites, radius)
    n0 = regions.launch_count()
    got = regions.nearest(mask.cuda() if dev is None else dev, sites, radius)
    _ran(n0, 2)
    bad = int((got.cpu() != want).sum())
    print(tuple(mask.shape), 'sites', sorted(sites)[:4], 'radius', radius, 'differing', bad, 'without a site', int((want < 0).sum()))
    assert got.dtype == torch.int32 and got.is_contiguous() and bad == 0
    return want


@pytest.mark.parametrize('size', [(5, 300), (300, 5), (4096, 70), (70, 4096)])
def test_nearest_on_rows_and_columns_longer_than_a_work_group(hip_lib, size):
    """Also the two limits: 4096 rows are 64 chunks of site words in pass 1 (its largest LDS image), 4096 columns the 16 KB row of pass 2."""
    mask = random_mask(1, size[0], size[1], 6, seed=size[0])[0]
    for radius in (-1, 7):
        _nearest_equal(mask, {2}, radius)


@pytest.mark.parametrize('radius', [0, 1, 3, 100, -1])
def test_nearest_at_every_radius(hip_lib, radius):
    mask = random_mask(1, 33, 70, 6, seed=11)[0]
    want = _nearest_equal(mask, {1, 5}, radius)
    assert radius != 100 or torch.equal(want, _nearest_equal(mask, {1, 5}, -1))          # radius 100 is larger than the image
    _nearest_equal(mask, set(), radius)
    _nearest_equal(mask, set(range(256)), radius)


def test_nearest_ties_along_the_bisector_and_a_pitched_view(hip_lib):
    mask = torch.zeros(40, 90, dtype=torch.uint8)
    mask[6, 10] = mask[33, 79] = 9                                              # two far-apart sites: a line of ties between them
    want = _nearest_equal(mask, {9}, -1)
    assert set(want.unique().tolist()) == {6 * 90 + 10, 33 * 90 + 79}
    mask[20, 10] = mask[6, 38] = 9                                              # and exact ties on a row and a column
    _nearest_equal(mask, {9}, -1)
    blobs = random_mask(1, 67, 131, 19, seed=12)[0]
    for shift in (1, 3):
        _nearest_equal(blobs, {0, 7, 18}, 9, dev=_view_in_canvas(blobs, shift))


def test_nearest_unbounded_at_frame_size(hip_lib):
    mask = random_mask(1, 512, 512, 6, seed=13)[0]
    mask[mask == 4] = 0
    mask[300, 17] = 4                                                           # one site: every pixel looks across the whole row
    _nearest_equal(mask, {4}, -1)
    _nearest_equal(mask, {1}, -1)


# ---- 3. warp ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def warp_case():
    mask = random_mask(1, 67, 131, 19, seed=14)[0]
    return mask, (mask % 3 == 0).to(torch.uint8), random_mask(1, 67, 131, 19, seed=15)[0]


MATRICES = {'identity': [[1, 0, 0], [0, 1, 0]], 'partly out of the image': [[1, 0, 90], [0, 1, -40]], 'rotation by 90 degrees': [[0, -1, 98], [1, 0, -32]],
            'scale x2': [[2, 0, -65], [0, 2, -33]], 'scale x1/2': [[0.5, 0, 32.5], [0, 0.5, 16.5]], 'shear and rotation': [[0.8, -0.5, 40.25], [0.3, 1.1, -9.75]]}


@pytest.mark.parametrize('name', sorted(MATRICES))
def test_warp_equals_the_cpu_formulation(hip_lib, warp_case, name):
    from pix2pix3d_amd import regions
    mask, region, under = warp_case
    coef = regions.affine_coef(MATRICES[name])
    want = regions.warp(mask, region, under, coef)
    assert name == 'identity' or not torch.equal(want, regions.warp(mask, region, under, regions.affine_coef(MATRICES['identity'])))
    n0 = regions.launch_count()
    got = regions.warp(mask.cuda(), region.cuda(), under.cuda(), coef)
    _ran(n0, 1)
    _bytes_apart(got, want.numpy(), name)


def test_warp_with_pitches_and_misaligned_pointers_inside_a_canvas(hip_lib, warp_case):
    """The pattern of test_odd_size_pitches_and_misaligned_pointers_inside_a_canvas: the bytes around the destination stay untouched."""
    from pix2pix3d_amd import regions
    mask, region, under = warp_case
    h, w = mask.shape
    coef = regions.affine_coef(MATRICES['shear and rotation'])
    want_inner = regions.warp(mask, region, under, coef).numpy()
    for shift in range(4):
        store = torch.full([(h + 5) * (w + 13) + 8], 171, dtype=torch.uint8, device='cuda')
        canvas = store[shift:shift + (h + 5) * (w + 13)].view(h + 5, w + 13)
        n0 = regions.launch_count()
        regions.warp(_view_in_canvas(mask, 3 - shift), _view_in_canvas(region, shift), _view_in_canvas(under, (shift + 1) % 4), coef,
                     out=canvas[2:2 + h, 5 + shift:5 + shift + w])
        _ran(n0, 1)
        want = np.full([h + 5, w + 13], 171, np.uint8)
        want[2:2 + h, 5 + shift:5 + shift + w] = want_inner
        got = canvas.cpu().numpy()
        assert np.array_equal(got, want), (shift, int((got != want).sum()))
        assert (store[:shift] == 171).all() and (store[shift + canvas.numel():] == 171).all()


# ---- 4. a session at seg2cat bench size ------------------------------------------------------------------------------------------------
def test_session_scales_one_label_removes_another_and_renders(bench_session):
    from pix2pix3d_amd import edit, regions
    G, s, u, base, pose = bench_session
    s.load(base, pose)                                                         # a fresh log on the fixture's session
    eye, ear = 4, 5
    c = Counters(G)
    try:
        n0 = regions.launch_count()
        s.scale(eye, 1.3)
        s.remove(ear)
        frame = s.render()
        torch.cuda.synchronize()
        assert c.take() == (1, 1, 1) and regions.launch_count() > n0             # Encoder and backbone once (and the MLP, for the seed's first w)
        box = regions.bbox(base == eye)
        cx, cy = (box[0] + box[2]) / 2, (box[1] + box[3]) / 2
        want = regions.transform(base, base == eye, [[1.3, 0, cx - 1.3 * cx], [0, 1.3, cy - 1.3 * cy]])
        want = regions.remove(want, ear)
        _bytes_apart(s.mask, want.numpy(), 'session mask')
        assert int((want != base).sum()) > 0 and int((want == ear).sum()) == 0 and tuple(frame['image'].shape) == (512, 512, 3)
        s.set_camera(yaw=40, pitch=52)
        s.render()
        assert c.take() == (0, 0, 0)                                          # a camera move runs neither
        n1 = regions.launch_count()
        s.undo(); s.undo()
        _bytes_apart(s.mask, base.numpy(), 'after two undos')
        assert regions.launch_count() == n1 and len(s.log) == 0
    finally:
        c.remove()
