"""pix2pix3d_amd.video on the device: the bytes of p3d_video_histogram / p3d_video_box_sums / p3d_video_quantize against the CPU formulation (integer
equality, the whole clip and one group per frame), at the smallest shapes that can go wrong: a pitched, offset window of a canvas written into a pitched
result; a strided selection of frames; every bin hit once (the whole LDS histogram and its flush); one colour (every add on one bin and one box); more
frames than there are work-group slots, so one work-group per frame; no frame at all; palettes with ties and of two rows."""
import numpy as np
import pytest
import torch

from model_cases import build_generator
from video_cases import gradient_frames, noise_frames, every_bin_once, decode_gif

pytestmark = pytest.mark.gpu


def _window(frames):
    """The frames as an offset, pitched window of a larger device canvas of other bytes."""
    f, h, w = frames.shape[:3]
    canvas = noise_frames(f + 1, h + 5, w + 7, seed=21).cuda()
    view = canvas[1:, 2:2 + h, 3:3 + w]
    view.copy_(frames)
    assert not view.is_contiguous() and view.data_ptr() != canvas.data_ptr()
    return view


def _single_colour():
    frames = torch.empty([2, 128, 160, 3], dtype=torch.uint8)
    frames[:] = torch.tensor([201, 17, 94], dtype=torch.uint8)
    return frames


CASES = {
    # name: (CPU frames, how they reach the device)
    'a window of a canvas': (lambda: torch.cat([gradient_frames(2, 37, 53, seed=22), noise_frames(1, 37, 53, seed=23)]), _window),
    'every second frame': (lambda: torch.cat([gradient_frames(4, 37, 53, seed=24), noise_frames(1, 37, 53, seed=25)]), lambda t: t.cuda()[::2]),
    'every bin once': (every_bin_once, lambda t: t.cuda()),
    'one colour': (_single_colour, lambda t: t.cuda()),
    'a work-group per frame': (lambda: noise_frames(600, 4, 5, seed=26), lambda t: t.cuda()),
}
_made = {}


def _case(name):
    """(CPU frames the device sees, bin -> box lookups [2][G, 32768], palettes, and the CPU results) — made once, then only read."""
    if name not in _made:
        from pix2pix3d_amd import video
        make, _ = CASES[name]
        frames = make()
        if name == 'every second frame':
            frames = frames[::2].contiguous()
        rng = np.random.default_rng(len(name))
        ref = {'frames': frames}
        for per_frame in (False, True):
            groups = frames.shape[0] if per_frame else 1
            lookup = torch.from_numpy(rng.integers(0, 256, size=[groups, 32768], dtype=np.uint8))
            palette = torch.from_numpy(rng.integers(0, 256, size=[groups, 200, 3], dtype=np.uint8))
            palette[:, 100:] = palette[:, :100]                                     # every row twice: ties everywhere
            n_colors = torch.from_numpy(rng.integers(1, 201, size=[groups]).astype(np.int32))
            n_colors[0] = 200
            args = (lookup, palette, n_colors) if per_frame else (lookup[0], palette[0], n_colors)
            ref[per_frame] = dict(args=args, counts=video.histogram(frames, per_frame), sums=video.box_sums(frames, args[0], per_frame),
                                  indices=video.quantize(frames, args[1], args[2], 16, per_frame))
        _made[name] = ref
    return _made[name]


def _device_frames(name):
    make, put = CASES[name]
    return put(make())


def _launches(fn, expected):
    from pix2pix3d_amd import video
    n0 = video.launch_count()
    out = fn()
    assert video.launch_count() == n0 + expected, (video.launch_count() - n0, expected)
    return out


@pytest.mark.parametrize('per_frame', [False, True])
@pytest.mark.parametrize('name', list(CASES))
def test_histogram_bytes_equal_the_cpu_formulation(hip_lib, name, per_frame):
    from pix2pix3d_amd import video
    ref, frames = _case(name), _device_frames(name)
    counts = _launches(lambda: video.histogram(frames, per_frame), 2)
    assert counts.is_cuda and counts.dtype == torch.int32 and torch.equal(counts.cpu(), ref[per_frame]['counts'])
    assert int(counts.sum()) == ref['frames'].numel() // 3
    if name == 'every bin once':
        assert (counts == 1).all()


@pytest.mark.parametrize('per_frame', [False, True])
@pytest.mark.parametrize('name', list(CASES))
def test_box_sums_bytes_equal_the_cpu_formulation(hip_lib, name, per_frame):
    from pix2pix3d_amd import video
    ref, frames = _case(name), _device_frames(name)
    sums = _launches(lambda: video.box_sums(frames, ref[per_frame]['args'][0].cuda(), per_frame), 2)
    assert sums.is_cuda and sums.dtype == torch.int64 and torch.equal(sums.cpu(), ref[per_frame]['sums'])
    assert int(sums[..., 3].sum()) == ref['frames'].numel() // 3


@pytest.mark.parametrize('per_frame', [False, True])
@pytest.mark.parametrize('name', list(CASES))
def test_quantize_bytes_equal_the_cpu_formulation(hip_lib, name, per_frame):
    from pix2pix3d_amd import video
    ref, frames = _case(name), _device_frames(name)
    _, palette, n_colors = ref[per_frame]['args']
    f, h, w = frames.shape[:3]
    canvas = torch.full([f, h + 3, w + 6], 251, dtype=torch.uint8, device='cuda')
    out = canvas[:, 1:1 + h, 5:5 + w]                                              # a pitched result at an odd byte offset
    got = _launches(lambda: video.quantize(frames, palette.cuda(), n_colors.cuda(), 16, per_frame, out=out), 1)
    assert got.data_ptr() == out.data_ptr() and torch.equal(out.cpu(), ref[per_frame]['indices'])
    out.fill_(251)
    assert (canvas == 251).all()                                                   # nothing around the window was written


@pytest.mark.parametrize('dither', [0, 64])
@pytest.mark.parametrize('rows', [2, 256])
def test_quantize_palettes_of_two_rows_and_of_256_with_ties(hip_lib, rows, dither):
    """256 rows on a coarse lattice (steps of 32, so many pixels sit exactly between two rows) with every colour twice; two rows equidistant from mid-grey."""
    from pix2pix3d_amd import video
    frames = torch.cat([gradient_frames(1, 37, 53, seed=27), noise_frames(1, 37, 53, seed=28)])
    frames[1, :8] = frames[1, :8] // 32 * 32 + 16                                   # exactly between lattice points on every channel
    frames[0, :4] = 128
    if rows == 2:
        palette = torch.tensor([[96, 128, 160], [160, 128, 96]], dtype=torch.uint8)
    else:
        palette = (torch.from_numpy(np.random.default_rng(29).integers(0, 8, size=[128, 3])) * 32).to(torch.uint8).repeat(2, 1)
    want = video.quantize(frames, palette, dither=dither)
    got = _launches(lambda: video.quantize(frames.cuda(), palette.cuda(), dither=dither), 1)
    assert torch.equal(got.cpu(), want)
    if rows == 256:
        assert int(want.max()) < 128                                                # the first of two equal rows
    elif dither == 0:
        assert (want[0, :4] == 0).all()


def test_no_frames_launch_nothing(hip_lib):
    from pix2pix3d_amd import video
    frames = torch.empty([0, 16, 16, 3], dtype=torch.uint8, device='cuda')
    palette = torch.zeros([4, 3], dtype=torch.uint8, device='cuda')
    counts = _launches(lambda: video.histogram(frames), 0)
    assert counts.is_cuda and tuple(counts.shape) == (32768,) and not counts.any()
    assert tuple(_launches(lambda: video.histogram(frames, True), 0).shape) == (0, 32768)
    assert not _launches(lambda: video.box_sums(frames, torch.zeros(32768, dtype=torch.uint8, device='cuda')), 0).any()
    assert tuple(_launches(lambda: video.quantize(frames, palette), 0).shape) == (0, 16, 16)


def test_the_entry_points_refuse_bad_arguments_before_any_launch(hip_lib):
    from pix2pix3d_amd import video, _lib
    frames = noise_frames(1, 8, 8).cuda()
    counts = torch.zeros([32768], dtype=torch.int32, device='cuda')
    lib, n0 = video.video_lib(), video.launch_count()
    stream = _lib.stream_of(frames)
    assert lib.p3d_video_histogram(_lib.ptr(frames), 192, 23, 1, 8, 8, 0, _lib.ptr(counts), stream) == _lib.P3D_ERR_ARGUMENT        # a row pitch under 3 w
    assert lib.p3d_video_histogram(_lib.ptr(frames), 0, 3 << 16, 2, 1 << 15, 1 << 15, 0, _lib.ptr(counts), stream) == _lib.P3D_ERR_ARGUMENT   # 2^31 pixels
    assert lib.p3d_video_histogram(_lib.ptr(frames), 192, 24, 1, 8, 8, 2, _lib.ptr(counts), stream) == _lib.P3D_ERR_ARGUMENT
    idx = torch.zeros([8, 8], dtype=torch.uint8, device='cuda')
    pal, n = torch.zeros([256, 3], dtype=torch.uint8, device='cuda'), torch.ones([1], dtype=torch.int32, device='cuda')
    for amplitude, row_pitch in ((65, 8), (-1, 8), (16, 7)):
        code = lib.p3d_video_quantize(_lib.ptr(frames), 192, 24, 1, 8, 8, 0, _lib.ptr(pal), _lib.ptr(n), amplitude, _lib.ptr(idx), 64, row_pitch, stream)
        assert code == _lib.P3D_ERR_ARGUMENT
    assert video.launch_count() == n0 and b'video_quantize' in lib.p3d_last_error()


@pytest.mark.parametrize('mode', ['global', 'frame'])
def test_palettize_on_the_device_equals_palettize_on_the_host(hip_lib, mode):
    from pix2pix3d_amd import video
    frames = gradient_frames(3, 64, 96, seed=30)
    want = video.palettize(frames, colors=256, dither=16, palette=mode)
    got = _launches(lambda: video.palettize(frames.cuda(), colors=256, dither=16, palette=mode), 5)
    for a, b in zip(got, want):
        assert a.is_cuda and a.dtype == b.dtype and torch.equal(a.cpu(), b)


def test_generate_video_writes_both_gifs_from_device_frames(hip_lib, tmp_path):
    from pix2pix3d_amd import views, video
    G = build_generator('seg2cat', 'cuda', depth=(64, 64))
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(41)).cuda()
    n0 = video.launch_count()
    out = views.generate_video(G, ws, 'seg2cat', str(tmp_path / 'v.gif'), str(tmp_path / 'l.gif'), n_frames=4, views_per_step=4, gif='device')
    assert video.launch_count() == n0 + 5 and out['image'].is_cuda                  # the image: five launches; the label video: none
    label, image = decode_gif(tmp_path / 'l.gif'), decode_gif(tmp_path / 'v.gif')
    assert all(any(np.array_equal(want, got) for got in label) for want in out['label'].cpu().numpy())
    if len(label) == 4:                                                            # (PIL merges frames that are identical)
        assert np.array_equal(label, out['label'].cpu().numpy())
    indices, palette, _ = video.palettize(out['image'], dither=16)
    assert np.array_equal(image, palette.cpu().numpy()[indices.cpu().numpy()])
