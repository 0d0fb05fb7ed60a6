"""pix2pix3d_amd.edit on the device: p3d_paint_strokes against the numpy oracle (0 differing bytes), p3d_label_features against the CPU module route (exact),
and one session at seg2cat bench size: encode against the CPU fp32 G.mapping, render against finish_frames(G.synthesis), what runs per event, launch counts."""
import copy

import numpy as np
import pytest
import torch

from conftest import rel_err, record_error
from model_cases import build_generator, replay_uniforms
from views_cases import numpy_scale, numpy_label, to_device_same_layout
from edit_cases import oracle_paint, random_strokes, random_mask, fromrgb_layer, module_features, Counters, demo_pose

pytestmark = pytest.mark.gpu


def _bytes_apart(a, ref, what):
    a = a.cpu().numpy()
    bad = int((a != ref).sum())
    print(what, 'differing bytes', bad, 'of', ref.size)
    assert a.shape == ref.shape and bad == 0, (what, bad)


# ---- 1. p3d_paint_strokes ------------------------------------------------------------------------------------------------------------
def test_300_strokes_at_frame_size_in_one_launch(hip_lib):
    """512^2, 300 strokes: more than one 256-stroke chunk, thicknesses 1 .. 60, endpoints inside and outside the canvas, many strokes over one tile."""
    from pix2pix3d_amd import edit, _lib
    base = random_mask(1, 512, 512, 6, seed=11)[0]
    strokes = random_strokes(300, 512, 512, 6, seed=12)
    strokes[40:60, 0:4] = np.array([250, 250, 262, 258]) + np.arange(20)[:, None]      # twenty strokes over the same tiles
    strokes[280:, 0:2] = [100, 400]                                                     # and a fan from one point in the second chunk
    n0 = _lib.launch_count()
    out = edit.paint_strokes(base.cuda(), strokes)
    torch.cuda.synchronize()
    assert _lib.launch_count() == n0 + 1
    ref = oracle_paint(base.numpy(), strokes)
    assert (ref != base.numpy()).mean() > 0.2
    _bytes_apart(out, ref, '512^2 x 300 strokes')


@pytest.mark.parametrize('k', [0, 1, 256, 257, 90])
def test_odd_size_pitches_and_misaligned_pointers_inside_a_canvas(hip_lib, k):
    """67 x 131 with source and destination row pitches != W and both pointers off by 1 .. 3 bytes (and aligned); the bytes around the destination stay untouched.
    K = 0 copies the base; 256 / 257 sit on the chunk boundary."""
    from pix2pix3d_amd import edit, _lib
    h, w = 67, 131
    base = random_mask(1, h, w, 19, seed=20 + k)[0]
    strokes = random_strokes(k, h, w, 19, seed=21 + k, t_max=25)
    ref = oracle_paint(base.numpy(), strokes)
    for shift in range(4):
        src_store = torch.full([(h + 2) * (w + 6) + 8], 77, dtype=torch.uint8)
        src = src_store[3 - shift:3 - shift + (h + 2) * (w + 6)].view(h + 2, w + 6)[1:1 + h, 2:2 + w]
        src.copy_(base)
        src_dev = to_device_same_layout(src)
        assert src_dev.stride(0) == w + 6 and src_dev.data_ptr() % 4 == (3 - shift + w + 6 + 2) % 4
        store = torch.full([(h + 5) * (w + 13) + 8], 171, dtype=torch.uint8, device='cuda')
        canvas = store[shift:shift + (h + 5) * (w + 13)].view(h + 5, w + 13)
        n0 = _lib.launch_count()
        edit.paint_strokes(src_dev, strokes, out=canvas[2:2 + h, 5 + shift:5 + shift + w])
        torch.cuda.synchronize()
        assert _lib.launch_count() == n0 + 1
        want = np.full([h + 5, w + 13], 171, np.uint8)
        want[2:2 + h, 5 + shift:5 + shift + w] = ref
        got = canvas.cpu().numpy()
        assert np.array_equal(got, want), (k, shift, int((got != want).sum()))
        assert (store[:shift] == 171).all() and (store[shift + canvas.numel():] == 171).all()


def test_paint_argument_errors_come_back_as_codes(hip_lib):
    m = torch.zeros(8, 8, dtype=torch.uint8, device='cuda')
    o = torch.zeros(8, 8, dtype=torch.uint8, device='cuda')
    assert hip_lib.p3d_paint_strokes(None, 8, o.data_ptr(), 8, 8, 8, None, 0, None) == -2 and b'non-null' in hip_lib.p3d_last_error()
    assert hip_lib.p3d_paint_strokes(m.data_ptr(), 8, o.data_ptr(), 8, 8, 4097, None, 0, None) == -2
    assert hip_lib.p3d_paint_strokes(m.data_ptr(), 8, o.data_ptr(), 8, 8, 8, None, 3, None) == -2 and b'no table' in hip_lib.p3d_last_error()
    assert hip_lib.p3d_paint_strokes(m.data_ptr(), 8, o.data_ptr(), 7, 8, 8, None, 0, None) == -2 and b'row pitch' in hip_lib.p3d_last_error()
    assert hip_lib.p3d_paint_strokes(m.data_ptr(), 8, m.data_ptr(), 8, 8, 8, None, 0, None) == -2 and b'out of place' in hip_lib.p3d_last_error()
    assert hip_lib.p3d_paint_strokes(m.data_ptr(), 8, o.data_ptr(), 8, 8, 8, None, 65536, None) == -2


# ---- 2. p3d_label_features -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def entry_cases():
    """{(L, size): (layer, mask with a byte 255 planted, CPU module result)} — computed once, never modified."""
    cases = {}
    for n_labels in (6, 19):
        layer = fromrgb_layer(n_labels, seed=n_labels)
        for n, h, w in ((2, 37, 41), (1, 512, 512)):
            mask = random_mask(n, h, w, n_labels, seed=h + n_labels)
            mask[n - 1, h // 3, w // 2] = 255
            cases[n_labels, (n, h, w)] = (layer, mask, module_features(layer, mask, n_labels))
    return cases


@pytest.mark.parametrize('fmt', [torch.contiguous_format, torch.channels_last], ids=['nchw', 'nhwc'])
@pytest.mark.parametrize('size', [(2, 37, 41), (1, 512, 512)])
@pytest.mark.parametrize('n_labels', [6, 19])
def test_label_features_equal_the_cpu_module_route(hip_lib, entry_cases, n_labels, size, fmt):
    from pix2pix3d_amd import edit, _lib
    layer, mask, want = entry_cases[n_labels, size]
    table = edit.label_table(layer, n_labels).cuda()
    for dtype in (torch.float32, torch.float16):
        n0 = _lib.launch_count()
        got = edit.label_features(mask.cuda(), table, dtype=dtype, memory_format=fmt)
        torch.cuda.synchronize()
        assert _lib.launch_count() == n0 + 1
        assert got.dtype == dtype and got.is_contiguous(memory_format=fmt) and tuple(got.shape) == tuple(want.shape)
        ref = want if dtype == torch.float32 else want.half()
        assert np.array_equal(got.cpu().numpy(), ref.numpy()), (n_labels, size, dtype, int((got.cpu() != ref).sum()))
    n, h, w = size
    assert torch.equal(got[n - 1, :, h // 3, w // 2].cpu(), table[n_labels].half().cpu())      # the planted byte reads row L


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_label_features_row_tails_and_mask_pitches_through_the_c_abi(hip_lib, dtype):
    """The planar kernel's row tail (W no multiple of the 16-byte pack, rows padded to one) and a mask that is a window of a larger one: only the C ABI can ask
    for these.  The bytes of the padding stay untouched."""
    from pix2pix3d_amd import edit, _lib
    n_labels, n, h, w, pad_w = 6, 2, 9, 43, 48
    layer = fromrgb_layer(n_labels, seed=3)
    big = random_mask(n, h + 3, w + 10, n_labels, seed=8)
    mask = to_device_same_layout(big[:, 2:2 + h, 7:7 + w])
    want = module_features(layer, big[:, 2:2 + h, 7:7 + w], n_labels)
    want = want if dtype == torch.float32 else want.half()
    table = edit.label_table(layer, n_labels).cuda()
    out = torch.full([n, 64, h, pad_w], -7.0, dtype=dtype, device='cuda')
    code = hip_lib.p3d_label_features(mask.data_ptr(), mask.stride(0), mask.stride(1), table.data_ptr(), n_labels, out.data_ptr(), _lib.DTYPE_CODE[dtype],
                                      _lib.i64x4(*out.stride()), n, 64, h, w, _lib.stream_of(out))
    torch.cuda.synchronize()
    assert code == 0, hip_lib.p3d_last_error()
    assert torch.equal(out[..., :w].cpu(), want) and bool((out[..., w:] == -7.0).all())
    assert hip_lib.p3d_label_features(mask.data_ptr(), mask.stride(0), mask.stride(1), table.data_ptr(), n_labels, out.data_ptr(), _lib.DTYPE_CODE[dtype],
                                      _lib.i64x4(*out.stride()), n, 66, h, w, None) == -2 and b'multiple of 4' in hip_lib.p3d_last_error()


# ---- 3. a session at seg2cat bench size ------------------------------------------------------------------------------------------------------
STROKES = [(150, 200, 230, 215, 35, 2), (230, 215, 300, 190, 35, 2), (260, 330, 260, 330, 50, 4), (100, 400, 420, 380, 9, 1)]


@pytest.fixture
def bench_session(hip_lib):
    """(G, a fresh session with a mask loaded and painted, draws, base, pose); the generator is built once."""
    from pix2pix3d_amd import edit
    G = build_generator('seg2cat', 'cuda', depth=(64, 64))
    g = torch.Generator().manual_seed(51)
    u = (torch.rand(1, 128 * 128, 64, 1, generator=g), torch.rand(128 * 128, 64, generator=g))
    base, pose = random_mask(1, 512, 512, 6, seed=52)[0], torch.from_numpy(demo_pose(G))
    s = edit.EditSession(G, cfg='seg2cat', seed=7, truncation_psi=0.75, jitter=u)
    s.load(base, pose)
    s.paint(STROKES)
    return G, s, u, base, pose


def test_encode_against_the_cpu_fp32_mapping(bench_session):
    """The session's ws (label entry + Encoder + cached MLP) and the device's one-hot G.mapping, both against the CPU fp32 G.mapping of the same weights, under the
    bound tests/test_model_api.py puts on the device's G.mapping."""
    from pix2pix3d_amd import edit
    G, s, u, base, pose = bench_session
    assert s.fast_entry and s.nrr == 128
    painted = torch.from_numpy(oracle_paint(base.numpy(), STROKES))
    _bytes_apart(s.mask, painted.numpy(), 'session mask')
    z = torch.from_numpy(np.random.RandomState(7).randn(1, G.z_dim).astype('float32'))
    fwd = edit.forward_label(G)
    with torch.no_grad():
        cpu_map = copy.deepcopy(G.backbone.mapping).cpu()
        want = cpu_map(z, G.mapping_label(fwd), {'mask': painted[None, None], 'pose': pose[None]}, truncation_psi=0.75).numpy()
        one_hot = G.mapping(z.cuda(), fwd.cuda(), {'mask': painted[None, None].cuda(), 'pose': pose[None].cuda()}, truncation_psi=0.75).cpu().numpy()
    ws = s.encode().cpu().numpy()
    errs = {'session': rel_err(ws, want), 'one_hot_route': rel_err(one_hot, want)}
    print('encode vs CPU fp32 G.mapping', errs)
    record_error('edit.encode.seg2cat', errs)
    assert ws.shape == want.shape and errs['session'] < 1e-3, errs


def test_render_equals_finish_frames_of_synthesis(bench_session):
    """Same ws, camera and draws: the session's frame (kept planes, use_cached_backbone) against finish_frames(G.synthesis(ws, c)) — the pair of routes, the statistic
    and the allowances of test_views_gpu.py's end-to-end comparison (fp16 heads: 1e-4 raw, 3e-3 after the heads, depth 1e-4); the session's bytes are exactly the
    numpy finishing of its own floats."""
    from pix2pix3d_amd import views, mesh
    G, s, u, base, pose = bench_session
    s.set_camera(yaw=70, pitch=48, roll=2)
    out = s.render(return_float=True)
    fl, ws, c = out['float'], s.encode(), s.camera
    with replay_uniforms(u[0], u[1]), torch.no_grad():
        one = G.synthesis(ws, c, neural_rendering_resolution=128, noise_mode='const')
    direct = views.finish_frames(one)
    errs = {k: rel_err(fl[k].float().cpu().numpy(), one[k].float().cpu().numpy()) for k in ('image_raw', 'semantic_raw', 'image', 'semantic')}
    errs['image_depth'] = float((fl['image_depth'] - one['image_depth']).abs().max())
    errs['image_bytes_apart'] = int((out['image'] != direct['image'][0]).sum())
    errs['label_index_apart'] = int((out['label_index'] != direct['label_index'][0]).sum())
    print('render vs finish_frames(G.synthesis)', errs)
    record_error('edit.render.seg2cat.fp16-sr', errs)
    assert errs['image_raw'] < 1e-4 and errs['semantic_raw'] < 1e-4 and errs['image_depth'] < 1e-4, errs
    assert errs['image'] < 3e-3 and errs['semantic'] < 3e-3, errs
    _bytes_apart(out['image'][None], numpy_scale(fl['image'].float().cpu().numpy(), -1.0, 1.0), 'image frame')
    colour, index = numpy_label(fl['semantic'].float().cpu().numpy(), mesh.default_palette(6).numpy())
    _bytes_apart(out['label'][None], colour, 'label frame')
    _bytes_apart(out['label_index'][None], index, 'label index')
    assert tuple(out['image'].shape) == (512, 512, 3) and out['image'].is_cuda and int(out['label_index'].max()) < 6


def test_events_run_only_their_stages_and_a_camera_move_launches_less(bench_session):
    from pix2pix3d_amd import _lib
    G, s, u, base, pose = bench_session
    s.render()
    c = Counters(G)
    try:
        s.paint([(300, 120, 340, 180, 21, 3)])
        n0 = _lib.launch_count()
        edited = s.render()
        torch.cuda.synchronize()
        n_edit = _lib.launch_count() - n0
        assert c.take() == (1, 0, 1)                                          # paint: Encoder once, MLP zero
        s.set_camera(yaw=35, pitch=55)
        n0 = _lib.launch_count()
        turned = s.render()
        torch.cuda.synchronize()
        n_camera = _lib.launch_count() - n0
        assert c.take() == (0, 0, 0)                                          # camera: neither, and no backbone
        print('launches: edit', n_edit, 'camera', n_camera)
        assert 0 < n_camera < n_edit and not torch.equal(turned['image'], edited['image'])
        s.set_seed(8)
        s.render()
        assert c.take() == (0, 1, 1)                                          # seed: MLP once, Encoder zero
        index = s.render()['label_index'].clone()
        s.take_view_as_mask()
        assert torch.equal(s.mask, index) and len(s.strokes) == 0
        s.undo()
        assert torch.equal(s.mask, index)
    finally:
        c.remove()
