"""pix2pix3d_amd.edit without a GPU: the numpy oracle of the stroke rule against first principles, the torch formulation against the oracle, every limit,
the demo's cameras, the label entry against the module route, and a whole session on a small CPU generator (values against G.mapping, what runs per event)."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from model_cases import build_generator
from edit_cases import oracle_paint, float_capsule, random_strokes, random_mask, fromrgb_layer, module_features, Counters, demo_pose

TOL = 5e-5                       # tests/test_model_api.py's CPU bound


# ---- 1. the oracle ---------------------------------------------------------------------------------------------------------------
def test_oracle_on_the_cases_one_can_check_by_hand():
    base = np.zeros([40, 50], np.uint8)
    out = oracle_paint(base, [(7, 11, 23, 11, 1, 3)])                      # t = 1, horizontal: exactly its row segment
    want = base.copy(); want[11, 7:24] = 3
    assert np.array_equal(out, want)
    out = oracle_paint(base, [(20, 15, 20, 15, 9, 2)])                      # zero length: the disc 4 r^2 <= t^2
    ys, xs = np.mgrid[0:40, 0:50]
    assert np.array_equal(out == 2, 4 * ((xs - 20) ** 2 + (ys - 15) ** 2) <= 81) and out.sum() > 0
    assert np.array_equal(oracle_paint(base + 5, [(-300, -200, -250, -220, 60, 1)]), base + 5)      # wholly off the canvas
    a, b = (5, 5, 45, 35, 7, 1), (5, 35, 45, 5, 7, 4)                         # crossing: the later label wins where both cover
    both = (oracle_paint(base, [a]) == 1) & (oracle_paint(base, [b]) == 4)
    assert both.sum() > 0 and (oracle_paint(base, [a, b])[both] == 4).all() and (oracle_paint(base, [b, a])[both] == 1).all()


def test_oracle_equals_the_float64_capsule_away_from_its_boundary():
    h, w = 96, 112
    strokes = random_strokes(200, h, w, 6, seed=3, t_max=40)
    left_out = 0
    for s in strokes:
        dist = float_capsule(h, w, s)
        sure = np.abs(dist) > 1e-9
        left_out += int((~sure).sum())
        got = oracle_paint(np.zeros([h, w], np.uint8), [tuple(s[:5]) + (1,)]) == 1
        assert np.array_equal(got[sure], (dist < 0)[sure]), s
    share = left_out / (len(strokes) * h * w)
    print('pixels within 1e-9 of a boundary:', left_out, 'share', share)
    assert share <= 1e-3


# ---- 2. the torch formulation and the limits ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('size,k', [((64, 64), 0), ((67, 131), 90), ((200, 160), 300)])
def test_cpu_paint_strokes_equals_the_oracle(size, k):
    from pix2pix3d_amd import edit
    h, w = size
    base = random_mask(1, h, w, 6, seed=k)[0]
    strokes = random_strokes(k, h, w, 6, seed=k + 1)
    out = edit.paint_strokes(base, strokes)
    bad = int((out.numpy() != oracle_paint(base.numpy(), strokes)).sum())
    print(size, k, 'differing bytes', bad)
    assert bad == 0 and out.data_ptr() != base.data_ptr()
    canvas = torch.full([h + 4, w + 9], 171, dtype=torch.uint8)                # out of place into a view of a larger canvas
    edit.paint_strokes(base, strokes, out=canvas[2:2 + h, 5:5 + w])
    want = np.full([h + 4, w + 9], 171, np.uint8); want[2:2 + h, 5:5 + w] = out.numpy()
    assert np.array_equal(canvas.numpy(), want)


def test_every_limit_is_a_value_error_before_any_launch():
    from pix2pix3d_amd import edit, _lib
    base = torch.zeros(32, 32, dtype=torch.uint8)
    n0 = _lib.launch_count()
    ok = [4, 4, 20, 20, 5, 1]
    for col, bad in ((4, 0), (4, 256), (5, 256), (5, -1), (0, -4097), (2, 8192), (1, -4097), (3, 8192)):
        s = list(ok); s[col] = bad
        with pytest.raises(ValueError):
            edit.paint_strokes(base, [s])
    for col, fine in ((4, 1), (4, 255), (5, 255), (0, -4096), (2, 8191)):
        s = list(ok); s[col] = fine
        edit.paint_strokes(base, [s])
    with pytest.raises(ValueError):
        edit.paint_strokes(base, np.tile(np.array([ok]), (65536, 1)))
    with pytest.raises(ValueError):
        edit.paint_strokes(torch.zeros(4097, 8, dtype=torch.uint8), [ok])
    with pytest.raises(ValueError):
        edit.paint_strokes(torch.zeros(8, 4097, dtype=torch.uint8), [ok])
    with pytest.raises(ValueError):
        edit.paint_strokes(base, [[1.5, 2, 3, 4, 5, 1]])
    with pytest.raises(ValueError):
        edit.paint_strokes(base.float(), [ok])
    with pytest.raises(ValueError):
        edit.paint_strokes(base, [ok], out=base)
    assert _lib.launch_count() == n0


# ---- 3. cameras ----------------------------------------------------------------------------------------------------------------
def test_camera_from_euler_is_the_demos_matrix():
    from scipy.spatial.transform import Rotation
    from pix2pix3d_amd import edit
    r = np.random.RandomState(0)
    worst = 0.0
    for roll, yaw, pitch in np.concatenate([r.uniform(-3, 3, [20, 3]), np.zeros([1, 3])]):
        m = Rotation.from_euler('zyx', [roll, yaw, pitch + np.pi], degrees=False).as_matrix()
        m = np.concatenate([m, np.array([[0, 0, 0]])], axis=0)
        m = np.concatenate([m, np.array([0, 0, 0, 1])[..., None]], axis=1)
        m[:3, 3] = -m[:3, 2] * 2.7
        got = edit.camera_from_euler(roll, yaw, pitch, 2.7)
        assert got.dtype == torch.float32 and tuple(got.shape) == (4, 4)
        worst = max(worst, float(np.abs(got.numpy().astype(np.float64) - m).max()))
    print('max abs difference', worst)
    assert worst <= 1e-6


def test_slider_units():
    from pix2pix3d_amd import edit
    assert edit.slider_angles(0, 0, 0) == (0.0, 0.0, 0.0)
    for yaw, pitch, roll in ((100, 50, 0), (-100, 100, 100)):
        got = edit.slider_angles(yaw=yaw, pitch=pitch, roll=roll)
        assert np.allclose(got, (roll / 100 * np.pi / 4, yaw / 100 * np.pi / 2, pitch / 100 * np.pi), rtol=0, atol=1e-15)
    assert np.allclose(edit.slider_angles(100, 100, 100), (np.pi / 4, np.pi / 2, np.pi))


# ---- 4. label entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_labels', [6, 19])
def test_label_features_equal_the_module_route_on_the_cpu(n_labels):
    from pix2pix3d_amd import edit
    layer = fromrgb_layer(n_labels, seed=n_labels)
    mask = random_mask(2, 37, 41, n_labels, seed=1)
    table = edit.label_table(layer, n_labels)
    assert tuple(table.shape) == (n_labels + 1, 64) and table.dtype == torch.float32
    got = edit.label_features(mask, table)
    assert torch.equal(got, module_features(layer, mask, n_labels))
    mask[1, 5, 7] = 255                                                      # a bad byte reads row L: the layer's answer to an all-zero pixel
    got = edit.label_features(mask, table)
    assert torch.equal(got[1, :, 5, 7], table[n_labels]) and torch.equal(got, module_features(layer, mask, n_labels))
    cl = edit.label_features(mask, table, dtype=torch.float16, memory_format=torch.channels_last)
    assert cl.dtype == torch.float16 and cl.stride(1) == 1 and torch.equal(cl, got.half())


def test_block_and_encoder_seams():
    from pix2pix3d_amd.training.networks_stylegan2 import DiscriminatorBlock
    from pix2pix3d_amd.training.triplane_cond import Encoder
    torch.manual_seed(0)
    enc = Encoder(img_resolution=32, img_channels=6, channel_base=1 / 64, model_kwargs={'num_ws': 7, 'w_dim': 16, 'output_mode': 'W+'}).eval().requires_grad_(False)
    img = torch.nn.functional.one_hot(random_mask(2, 32, 32, 6, seed=2).long(), 6).permute(0, 3, 1, 2).float()
    with torch.no_grad():
        want = enc(img)['ws']
        got = enc(None, entry_features=enc.b32.fromrgb(img))['ws']
    assert torch.equal(got, want)
    skip = DiscriminatorBlock(0, 8, 8, resolution=32, img_channels=6, first_layer_idx=0, architecture='skip')
    with pytest.raises(ValueError):
        skip(None, img, feats=torch.zeros(2, 8, 32, 32))
    inner = DiscriminatorBlock(8, 8, 8, resolution=32, img_channels=6, first_layer_idx=0, architecture='resnet')
    with pytest.raises(ValueError):
        inner(torch.zeros(2, 8, 32, 32), None, feats=torch.zeros(2, 8, 32, 32))


# ---- 5. a session on a CPU generator ---------------------------------------------------------------------------------------------
def _small():
    return build_generator('seg2cat', 'cpu', cbase=2048, cmax=32, depth=(6, 6), sr_num_fp16_res=0)


@pytest.fixture(scope='module')
def loaded():
    """(G, res, base mask, pose): shared, never modified."""
    G = _small()
    res = G.backbone.mapping.in_resolution
    return G, res, random_mask(1, res, res, 6, seed=4)[0], torch.from_numpy(demo_pose(G))


def test_encode_equals_g_mapping_through_the_one_hot_route(loaded):
    from pix2pix3d_amd import edit
    G, res, base, pose = loaded
    s = edit.EditSession(G, seed=3, truncation_psi=0.7, neural_rendering_resolution=16)
    assert s.fast_entry
    s.load(base, pose)
    strokes = random_strokes(12, res, res, 6, seed=5)
    s.paint(strokes)
    ws = s.encode()
    z = torch.from_numpy(np.random.RandomState(3).randn(1, G.z_dim).astype('float32'))
    painted = torch.from_numpy(oracle_paint(base.numpy(), strokes))
    assert torch.equal(s.mask, painted)
    with torch.no_grad():
        want = G.mapping(z, edit.forward_label(G), {'mask': painted[None, None], 'pose': pose[None]}, truncation_psi=0.7)
    err = rel_err(ws.numpy(), want.numpy())
    print('encode vs G.mapping rel_err', err)
    assert tuple(ws.shape) == tuple(want.shape) and err < TOL


def test_each_event_runs_only_the_stages_its_input_reaches(loaded):
    from pix2pix3d_amd import edit
    G, res, base, pose = loaded
    s = edit.EditSession(G, seed=1, neural_rendering_resolution=16, hold_texture=False)
    c = Counters(G)
    try:
        s.load(base, pose)
        first = s.render()
        assert c.take() == (1, 1, 1)
        assert tuple(first['image'].shape) == (res, res, 3) and tuple(first['label'].shape) == (res, res, 3) and tuple(first['label_index'].shape) == (res, res)
        assert all(v.dtype == torch.uint8 for v in first.values())
        s.render()
        assert c.take() == (0, 0, 0)                                          # nothing changed: nothing runs
        s.paint([(res // 4, res // 3, res // 2, res // 2, 35, 2)])
        edited = s.render()
        assert c.take() == (1, 0, 1)                                          # paint: Encoder once, MLP zero
        assert not torch.equal(edited['image'], first['image'])
        s.set_camera(yaw=60, pitch=45, roll=3)
        turned = s.render()
        assert c.take() == (0, 0, 0)                                          # camera: neither, and no backbone
        assert not torch.equal(turned['image'], edited['image'])
        s.set_seed(2)
        s.render()
        assert c.take() == (0, 1, 1)                                          # seed: MLP once, Encoder zero
        s.set_seed(1)
        s.render()
        assert c.take() == (0, 0, 1)                                          # a seed seen before: its w is kept
        host = s.frame()
        assert c.take() == (0, 0, 0) and isinstance(host['image'], np.ndarray) and np.array_equal(host['label_index'], s.render()['label_index'].numpy())
    finally:
        c.remove()


def test_undo_clear_and_the_cross_view_edit(loaded, tmp_path):
    from PIL import Image
    from pix2pix3d_amd import edit
    G, res, base, pose = loaded
    s = edit.EditSession(G, neural_rendering_resolution=16)
    with pytest.raises(RuntimeError):
        s.mask
    s.load(base.numpy(), pose.numpy())
    assert torch.equal(s.mask, base)
    a, b = [(10, 10, res - 10, res - 20, 9, 1)], [(res - 10, 10, 10, res - 20, 9, 5), (res // 2, 0, res // 2, res, 3, 0)]
    s.paint(a)
    one = s.mask.clone()
    s.paint(b)
    assert torch.equal(s.mask, torch.from_numpy(oracle_paint(base.numpy(), a + b))) and len(s.strokes) == 3
    s.undo()
    assert torch.equal(s.mask, one)                                           # one call = one undo step
    s.undo(); s.undo()
    assert torch.equal(s.mask, base) and len(s.strokes) == 0
    s.paint(a); s.clear()
    assert torch.equal(s.mask, base)
    with pytest.raises(ValueError):
        s.paint([(1, 1, 5, 5, 3, 6)])                                          # label 6 in a six-label mask
    with pytest.raises(ValueError):
        s.load(base + 6, pose)
    s.paint(a)
    s.set_camera(yaw=80, pitch=50)
    index = s.render()['label_index'].clone()
    s.take_view_as_mask()
    assert torch.equal(s.mask, index) and len(s.strokes) == 0 and int(s.mask.max()) < 6
    s.paint(b)
    assert torch.equal(s.mask, torch.from_numpy(oracle_paint(index.numpy(), b)))
    s.save(str(tmp_path / 'ui'))
    with Image.open(tmp_path / 'ui' / 'mask.png') as im:
        assert np.array_equal(np.asarray(im), s.mask.numpy())
    with Image.open(tmp_path / 'ui' / 'mask_color.png') as im:
        assert np.array_equal(np.asarray(im), s.palette[s.mask.long()].numpy())
    with Image.open(tmp_path / 'ui' / 'output.png') as im:
        assert np.array_equal(np.asarray(im), s.render()['image'].numpy())


def test_held_texture_and_replay_order(loaded):
    from pix2pix3d_amd import edit
    G, res, base, pose = loaded
    s = edit.EditSession(G, seed=1, neural_rendering_resolution=16)             # hold_texture=True
    s.load(base, pose)
    first = s.encode().clone()
    s.set_seed(2)
    second = s.encode().clone()
    assert torch.equal(second[:, 8:], first[:, 8:]) and not torch.equal(second[:, 7], first[:, 7]) and torch.equal(second[:, :7], first[:, :7])
    s.clear_texture()
    third = s.encode()
    assert not torch.equal(third[:, 8:], first[:, 8:]) and torch.equal(third[:, 7:8].expand(-1, third.shape[1] - 8, -1), third[:, 8:])
    a, b = (10, 10, res - 10, res - 10, 11, 4), (res - 10, 10, 10, res - 10, 11, 1)      # crossing; drawn label 4 first
    by_time, by_label = edit.EditSession(G, neural_rendering_resolution=16), edit.EditSession(G, neural_rendering_resolution=16, replay='label')
    for t in (by_time, by_label):
        t.load(base, pose)
        t.paint([a]); t.paint([b])
    assert torch.equal(by_time.mask, torch.from_numpy(oracle_paint(base.numpy(), [a, b])))
    assert torch.equal(by_label.mask, torch.from_numpy(oracle_paint(base.numpy(), [b, a])))
    assert not torch.equal(by_time.mask, by_label.mask)
    with pytest.raises(ValueError):
        edit.EditSession(G, replay='colour')
