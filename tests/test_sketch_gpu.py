"""pix2pix3d_amd.sketch on the device: the bytes of p3d_sketch_condition / _edge_classes / _link / _thin_step against the CPU formulation (integer equality and
float bits, the library's own launch counter moving as the header states), argument errors before any launch, and a device session on a small edge2car generator."""
import numpy as np
import pytest
import torch

from model_cases import build_generator, replay_uniforms
from views_cases import to_device_same_layout
from edit_cases import Counters, demo_pose
from sketch_cases import scene, random_grey, random_rgb, crossing_lines, pitched_view

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 16, 64                                # P3D_SKETCH_TILE_H / _W (asserted below); the one-pixel kernels' groups are 4 x 64


def _grey_cases():
    """Grey images at the smallest shapes that can go wrong: single rows and columns, one pixel past the work-group tile in each direction, lines through
    the tiles' corners, constant images."""
    return {'1x1': random_grey(1, 1, 1), '1x64': random_grey(1, 64, 2), '64x1': random_grey(64, 1, 3), '2x2': random_grey(2, 2, 4),
            'tile+1': random_grey(TILE_H + 1, TILE_W + 1, 5), '37x53': random_grey(37, 53, 6), 'corners': crossing_lines(2 * TILE_H + 8, 2 * TILE_W + 12),
            'zeros': torch.zeros(19, 70, dtype=torch.uint8), 'full': torch.full([19, 70], 255, dtype=torch.uint8)}


def _rgb_of(name, grey):
    if name in ('zeros', 'full', 'corners'):
        return torch.stack([grey, grey, grey], dim=2).contiguous()
    return random_rgb(grey.shape[0], grey.shape[1], seed=40 + grey.shape[1])


NAMES = sorted(_grey_cases())


@pytest.fixture(scope='module')
def refs():
    """Every CPU result the byte tests compare with — computed once, never modified."""
    from pix2pix3d_amd import sketch
    assert (sketch.TILE_H, sketch.TILE_W) == (TILE_H, TILE_W)
    r = {'grey': _grey_cases()}
    r['rgb'] = {n: _rgb_of(n, g) for n, g in r['grey'].items()}
    r['condition'] = {(n, res, blur, conv): sketch.condition(g, res, blur=blur, table=conv)
                      for n, g in r['grey'].items() for res in (16, 65) for blur in (True, False) for conv in ('dataset', 'input')}
    r['classes'] = {(n, kind, smooth): sketch.edge_classes(r[kind][n], 60, 240, smooth=smooth) for n in r['grey'] for kind in ('rgb', 'grey') for smooth in (True, False)}
    r['link'] = {n: sketch.link(c) for (n, kind, smooth), c in r['classes'].items() if kind == 'grey' and not smooth}
    r['thin_step'] = {(n, step): sketch.thin_step(g, 100, step) for n, g in r['grey'].items() for step in (0, 1)}
    r['thin'] = {n: sketch.thin(g, 100, 2) for n, g in r['grey'].items()}
    return r


def _ran(n0, launches):
    from pix2pix3d_amd import sketch
    torch.cuda.synchronize()
    assert sketch.launch_count() == n0 + launches, (sketch.launch_count() - n0, launches)


def _same(got, want, what):
    bad = int((got.cpu() != want).sum())
    print(what, 'differing', bad, 'of', want.numel())
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape) and got.is_cuda and bad == 0, (what, bad)


# ---- 1. bytes of every entry point ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_condition_equals_the_cpu_formulation(hip_lib, refs, name):
    from pix2pix3d_amd import sketch
    ink = refs['grey'][name].cuda()
    for (n, res, blur, conv), want in refs['condition'].items():
        if n == name:
            n0 = sketch.launch_count()
            got = sketch.condition(ink, res, blur=blur, table=conv)
            _ran(n0, 1)
            _same(got.view(torch.int32), want.view(torch.int32), f'condition {name} -> {res} blur={blur} {conv}')


@pytest.mark.parametrize('smooth', [True, False], ids=['smooth', 'raw'])
@pytest.mark.parametrize('kind', ['rgb', 'grey'])
@pytest.mark.parametrize('name', NAMES)
def test_edge_classes_equal_the_cpu_formulation(hip_lib, refs, name, kind, smooth):
    from pix2pix3d_amd import sketch
    want = refs['classes'][name, kind, smooth]
    n0 = sketch.launch_count()
    got = sketch.edge_classes(refs[kind][name].cuda(), 60, 240, smooth=smooth)
    _ran(n0, 1)
    print(name, kind, smooth, 'weak', int((want == 1).sum()), 'strong', int((want == 2).sum()))
    _same(got, want, f'edge_classes {name} {kind} smooth={smooth}')


@pytest.mark.parametrize('name', NAMES)
def test_link_equals_the_cpu_formulation(hip_lib, refs, name):
    from pix2pix3d_amd import sketch, regions
    classes = refs['classes'][name, 'grey', False]
    n0, r0 = sketch.launch_count(), regions.launch_count()
    got = sketch.link(classes.cuda())
    _ran(n0, 2)
    assert regions.launch_count() == r0 + 3                                    # the components are p3d_label_components: no second union-find
    _same(got, refs['link'][name], f'link {name}')


@pytest.mark.parametrize('name', NAMES)
def test_thinning_equals_the_cpu_formulation(hip_lib, refs, name):
    from pix2pix3d_amd import sketch
    ink = refs['grey'][name].cuda()
    for step in (0, 1):
        n0 = sketch.launch_count()
        got = sketch.thin_step(ink, 100, step)
        _ran(n0, 1)
        _same(got, refs['thin_step'][name, step], f'thin_step {name} step {step}')
    n0 = sketch.launch_count()
    got = sketch.thin(ink, 100, 2)
    _ran(n0, 4)
    _same(got, refs['thin'][name], f'thin {name}')
    assert torch.equal(ink.cpu(), refs['grey'][name])                          # the caller's canvas is never a destination


def test_hysteresis_and_edges_of_the_scene(hip_lib):
    from pix2pix3d_amd import sketch
    rgb = scene()
    want_classes = sketch.edge_classes(rgb, 40, 120)
    want = sketch.link(want_classes)
    assert int(((want_classes == 1) & (want == 255)).sum()) >= 1 and int(((want_classes == 1) & (want == 0)).sum()) >= 1
    _same(sketch.edges(rgb.cuda(), 40, 120), want, 'edges of the scene')


# ---- 2. a window of a pitched canvas, written into a pitched result ---------------------------------------------------------------------------
def _canvas_result(h, w, shift):
    store = torch.full([(h + 5) * (w + 13) + 8], 171, dtype=torch.uint8, device='cuda')
    canvas = store[shift:shift + (h + 5) * (w + 13)].view(h + 5, w + 13)
    return store, canvas, canvas[2:2 + h, 5 + shift:5 + shift + w]


def _untouched(store, canvas, shift, want_inner):
    h, w = want_inner.shape
    want = np.full(tuple(canvas.shape), 171, np.uint8)
    want[2:2 + h, 5 + shift:5 + shift + w] = want_inner.numpy()
    got = canvas.cpu().numpy()
    assert np.array_equal(got, want), (shift, int((got != want).sum()))
    assert (store[:shift] == 171).all() and (store[shift + canvas.numel():] == 171).all()


@pytest.mark.parametrize('shift', [1, 2, 3])
def test_windows_of_pitched_canvases_and_untouched_surroundings(hip_lib, refs, shift):
    """37 x 53 at an odd offset inside a canvas of other bytes (row pitch W + 6 pixels), into a window of a canvas of 171s."""
    from pix2pix3d_amd import sketch, _lib
    grey, rgb = refs['grey']['37x53'], refs['rgb']['37x53']
    h, w = grey.shape
    grey_dev, rgb_dev = to_device_same_layout(pitched_view(grey, shift)), to_device_same_layout(pitched_view(rgb, shift))
    assert grey_dev.stride(0) == w + 6 and rgb_dev.stride(0) == 3 * (w + 6) and torch.equal(rgb_dev.cpu(), rgb)
    for kind, image in (('rgb', rgb_dev), ('grey', grey_dev)):
        for smooth in (True, False):
            store, canvas, window = _canvas_result(h, w, shift)
            sketch.edge_classes(image, 60, 240, smooth=smooth, out=window)
            _untouched(store, canvas, shift, refs['classes']['37x53', kind, smooth])
    classes = to_device_same_layout(pitched_view(refs['classes']['37x53', 'grey', False], shift))
    store, canvas, window = _canvas_result(h, w, shift)
    sketch.link(classes, out=window)
    _untouched(store, canvas, shift, refs['link']['37x53'])
    for step in (0, 1):
        store, canvas, window = _canvas_result(h, w, shift)
        sketch.thin_step(grey_dev, 100, step, out=window)
        _untouched(store, canvas, shift, refs['thin_step']['37x53', step])
    # the conditioning image with a row pitch: only the C ABI can ask for it
    res, table = 16, sketch.condition_table('dataset').cuda()
    out = torch.full([res + 2, res + 7], -7.0, dtype=torch.float32, device='cuda')
    window = out[1:1 + res, 3:3 + res]
    code = sketch.sketch_lib().p3d_sketch_condition(grey_dev.data_ptr(), grey_dev.stride(0), h, w, 1, table.data_ptr(), window.data_ptr(), window.stride(0), res,
                                                    _lib.stream_of(out))
    torch.cuda.synchronize()
    assert code == 0, sketch.sketch_lib().p3d_last_error()
    want = torch.full([res + 2, res + 7], -7.0)
    want[1:1 + res, 3:3 + res] = refs['condition']['37x53', res, True, 'dataset'][0, 0]
    assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32))


# ---- 3. launches and arguments ---------------------------------------------------------------------------------------------------------------
def test_zero_size_images_launch_nothing(hip_lib):
    from pix2pix3d_amd import sketch, regions
    n0, r0 = sketch.launch_count(), regions.launch_count()
    for shape in ((0, 5), (5, 0)):
        empty = torch.zeros(shape, dtype=torch.uint8, device='cuda')
        assert tuple(sketch.thin(empty).shape) == shape and tuple(sketch.link(empty).shape) == shape and tuple(sketch.edge_classes(empty, 1, 2).shape) == shape
        assert tuple(sketch.edges(torch.zeros(shape + (3,), dtype=torch.uint8, device='cuda'), 1, 2).shape) == shape
        assert sketch.condition(empty, 16).numel() == 0 and sketch.condition(empty, 16).is_cuda
    assert sketch.condition(torch.zeros(4, 4, dtype=torch.uint8, device='cuda'), 0).numel() == 0
    _ran(n0, 0)
    assert regions.launch_count() == r0


def test_argument_errors_come_back_as_codes_before_any_launch(hip_lib):
    from pix2pix3d_amd import sketch, _lib
    lib = sketch.sketch_lib()
    a = torch.zeros(8, 8, dtype=torch.uint8, device='cuda')
    o = torch.zeros(8, 8, dtype=torch.uint8, device='cuda')
    ids = torch.zeros(8, 8, dtype=torch.int32, device='cuda')
    flag = torch.zeros(64, dtype=torch.int32, device='cuda')
    table, f = sketch.condition_table().cuda(), torch.zeros(8, 8, device='cuda')
    bad = _lib.P3D_ERR_ARGUMENT
    n0 = sketch.launch_count()

    def said(name):
        return name in lib.p3d_last_error()

    assert lib.p3d_sketch_condition(a.data_ptr(), 7, 8, 8, 1, table.data_ptr(), f.data_ptr(), 8, 8, None) == bad and said(b'sketch_condition') and said(b'row pitch')
    assert lib.p3d_sketch_condition(a.data_ptr(), 8, 8, 8, 1, table.data_ptr(), f.data_ptr(), 7, 8, None) == bad and said(b'row pitch')
    assert lib.p3d_sketch_condition(a.data_ptr(), 8, 8, 8, 1, table.data_ptr(), f.data_ptr(), 8, 0, None) == bad and said(b'resolution')
    assert lib.p3d_sketch_condition(a.data_ptr(), 8, 8, 4097, 1, table.data_ptr(), f.data_ptr(), 8, 8, None) == bad
    assert lib.p3d_sketch_edge_classes(a.data_ptr(), 7, 1, o.data_ptr(), 8, 8, 8, 1, 2, 1, None) == bad and said(b'sketch_edge_classes') and said(b'row pitch')
    assert lib.p3d_sketch_edge_classes(a.data_ptr(), 23, 3, o.data_ptr(), 8, 8, 8, 1, 2, 1, None) == bad and said(b'row pitch')
    assert lib.p3d_sketch_edge_classes(a.data_ptr(), 8, 1, o.data_ptr(), 8, 8, 8, 3, 2, 1, None) == bad and said(b'low <= high')
    assert lib.p3d_sketch_edge_classes(a.data_ptr(), 8, 1, o.data_ptr(), 8, 8, 8, 1, 2041, 1, None) == bad and said(b'2040')
    assert lib.p3d_sketch_edge_classes(a.data_ptr(), 8, 2, o.data_ptr(), 8, 8, 8, 1, 2, 1, None) == bad and said(b'channels')
    assert lib.p3d_sketch_link(a.data_ptr(), 7, ids.data_ptr(), flag.data_ptr(), o.data_ptr(), 8, 8, 8, None) == bad and said(b'sketch_link')
    assert lib.p3d_sketch_link(a.data_ptr(), 8, ids.data_ptr(), None, o.data_ptr(), 8, 8, 8, None) == bad and said(b'non-null')
    assert lib.p3d_sketch_thin_step(a.data_ptr(), 8, o.data_ptr(), 7, 8, 8, 100, 0, None) == bad and said(b'sketch_thin_step') and said(b'row pitch')
    assert lib.p3d_sketch_thin_step(a.data_ptr(), 8, o.data_ptr(), 8, 8, 8, 100, 2, None) == bad and said(b'step')
    assert lib.p3d_sketch_thin_step(a.data_ptr(), 8, o.data_ptr(), 8, 8, 8, 100, -1, None) == bad
    assert lib.p3d_sketch_thin_step(a.data_ptr(), 8, o.data_ptr(), 8, 8, 8, 0, 0, None) == bad and said(b'threshold')
    assert lib.p3d_sketch_thin_step(a.data_ptr(), 8, a.data_ptr(), 8, 8, 8, 100, 0, None) == bad and said(b'out of place')
    _ran(n0, 0)


# ---- 4. a device session on a small edge2car generator ----------------------------------------------------------------------------------------
@pytest.fixture
def small_session(hip_lib):
    """(G, a fresh session with a canvas loaded and drawn on, draws); the generator is built once."""
    from pix2pix3d_amd import sketch
    G = build_generator('edge2car', 'cuda', cbase=2048, cmax=32, depth=(8, 8), sr_num_fp16_res=0)
    g = torch.Generator().manual_seed(61)
    u = (torch.rand(1, 64 * 64, 8, 1, generator=g), torch.rand(64 * 64, 8, generator=g))
    s = sketch.SketchSession(G, cfg='edge2car', seed=5, truncation_psi=0.8, jitter=u)
    s.load(crossing_lines(300, 260, step=40), torch.from_numpy(demo_pose(G)))
    s.pen([(30, 30, 220, 250, 3), (220, 250, 40, 200, 1)])
    return G, s, u


def test_session_canvas_and_condition_equal_the_cpu_formulation(small_session):
    from pix2pix3d_amd import sketch, edit
    G, s, u = small_session
    want = edit.paint_strokes(crossing_lines(300, 260, step=40), [(30, 30, 220, 250, 3, 255), (220, 250, 40, 200, 1, 255)])
    _same(s.canvas, want, 'session canvas')
    n0 = sketch.launch_count()
    got = s.condition()
    _ran(n0, 1)
    assert s.condition() is got
    _ran(n0, 1)
    _same(got.view(torch.int32), sketch.condition(want, 128).view(torch.int32), 'session condition')
    s.undo(); s.erase([(0, 150, 259, 150, 11)])                                # an entry replaced with no read in between: the kept canvas is no prefix
    want = edit.paint_strokes(crossing_lines(300, 260, step=40), [(0, 150, 259, 150, 11, 0)])
    _same(s.canvas, want, 'session canvas after undo and erase')
    _same(s.condition().view(torch.int32), sketch.condition(want, 128).view(torch.int32), 'session condition after undo and erase')
    s.clear(); s.pen([(5, 5, 250, 290, 1)])
    _same(s.canvas, edit.paint_strokes(crossing_lines(300, 260, step=40), [(5, 5, 250, 290, 1, 255)]), 'session canvas after clear and pen')


def test_session_render_equals_finish_frames_of_synthesis(small_session):
    from pix2pix3d_amd import views
    G, s, u = small_session
    s.set_camera(yaw=60, pitch=45, roll=1)
    out, ws, c = s.render(), s.encode(), s.camera
    with replay_uniforms(u[0], u[1]), torch.no_grad():
        one = G.synthesis(ws, c, neural_rendering_resolution=64, noise_mode='const')
    direct = views.finish_frames(one, label_mode='grey')
    apart = {k: int((out[k] != direct[k][0]).sum()) for k in ('image', 'label')}
    print('render vs finish_frames(G.synthesis): differing bytes', apart)
    assert tuple(out['image'].shape) == (128, 128, 3) and tuple(out['label'].shape) == (128, 128) and out['image'].is_cuda and sorted(out) == ['image', 'label']
    assert apart == {'image': 0, 'label': 0}


def test_session_events_run_only_their_stages(small_session):
    from pix2pix3d_amd import _lib, sketch
    G, s, u = small_session
    s.render()
    c = Counters(G)
    try:
        s.pen([(100, 20, 110, 280, 5)])
        n0, k0 = _lib.launch_count(), sketch.launch_count()
        edited = s.render()
        torch.cuda.synchronize()
        n_edit = _lib.launch_count() - n0
        assert c.take() == (1, 1, 1) and sketch.launch_count() == k0 + 1        # a pen call: one conditioning launch, G.mapping (Encoder and MLP) and the backbone once
        s.set_camera(yaw=35, pitch=55)
        n0, k0 = _lib.launch_count(), sketch.launch_count()
        turned = s.render()
        torch.cuda.synchronize()
        n_camera = _lib.launch_count() - n0
        assert c.take() == (0, 0, 0) and sketch.launch_count() == k0            # a camera move: neither Encoder nor backbone, and no canvas work
        print('launches: edit', n_edit, 'camera', n_camera)
        assert 0 < n_camera < n_edit and not torch.equal(turned['image'], edited['image'])
        s.erase([(100, 20, 110, 280, 9)])
        s.undo()
        s.render()
        assert c.take() == (1, 1, 1)
    finally:
        c.remove()


def test_session_takes_the_view_back_as_a_traced_canvas(small_session):
    from pix2pix3d_amd import sketch
    G, s, u = small_session
    label = s.render()['label'].clone()
    n0 = sketch.launch_count()
    s.take_view_as_canvas()
    canvas = s.canvas
    _ran(n0, 4)
    assert canvas.is_cuda and canvas.dtype == torch.uint8 and set(canvas.unique().tolist()) <= {0, 255} and len(s.log) == 0
    _same(canvas, sketch.trace(255 - label.cpu()), 'canvas after take_view_as_canvas')
    s.undo()
    assert torch.equal(s.canvas, canvas)
