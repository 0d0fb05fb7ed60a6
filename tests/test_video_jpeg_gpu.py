"""pix2pix3d_amd.video's JPEG kernels on the device: the bytes of p3d_video_jpeg_blocks and p3d_video_jpeg_scan against the CPU formulation (integer
equality) and the launch counts p3d_video.h states, at the smallest shapes that can go wrong: a pitched, offset window of a canvas; a strided selection of
frames; pictures smaller than an MCU; one colour (every block a DC code and EOB); noise at quality 100 (the longest codes, byte stuffing); one interval per
frame over many frames; MCU counts that are no multiple of the restart interval; more than eight intervals a frame (RSTm wraps); no frame at all."""
import ctypes
import warnings

import pytest
import torch

from jpeg_cases import SUBSAMPLINGS, random_coefficients
from video_cases import gradient_frames, noise_frames

pytestmark = pytest.mark.gpu


def _window(frames):
    """The frames as an offset, pitched window of a larger device canvas of other bytes."""
    f, h, w = frames.shape[:3]
    canvas = noise_frames(f + 1, h + 5, w + 7, seed=51).cuda()
    view = canvas[1:, 2:2 + h, 3:3 + w]
    view.copy_(frames)
    assert not view.is_contiguous() and view.data_ptr() != canvas.data_ptr()
    return view


def _single_colour():
    frames = torch.empty([2, 128, 160, 3], dtype=torch.uint8)
    frames[:] = torch.tensor([201, 17, 94], dtype=torch.uint8)
    return frames


CASES = {
    # name: (CPU frames, how they reach the device, quality)
    'a window of a canvas': (lambda: torch.cat([gradient_frames(2, 37, 53, seed=52), noise_frames(1, 37, 53, seed=53)]), _window, 90),
    'every second frame': (lambda: torch.cat([gradient_frames(4, 37, 53, seed=54), noise_frames(1, 37, 53, seed=55)]), lambda t: t.cuda()[::2], 75),
    'one pixel': (lambda: noise_frames(1, 1, 1, seed=56), lambda t: t.cuda(), 90),
    'below one MCU': (lambda: noise_frames(2, 7, 9, seed=57), lambda t: t.cuda(), 90),
    'one colour': (_single_colour, lambda t: t.cuda(), 90),
    'noise at quality 100': (lambda: noise_frames(2, 24, 40, seed=58), lambda t: t.cuda(), 100),
    'an interval per frame': (lambda: noise_frames(600, 8, 8, seed=59), lambda t: t.cuda(), 50),
    'a last interval of three MCUs': (lambda: gradient_frames(1, 24, 200, seed=60, noise=20), lambda t: t.cuda(), 95),      # 75 MCUs at 4:4:4, 26 at 4:2:0
    'ten intervals a frame': (lambda: gradient_frames(2, 16, 1200, seed=61, noise=12), lambda t: t.cuda(), 90),           # 300 / 75 MCUs: 38 / 10 intervals
}
_made = {}


def _case(name, subsampling):
    """(CPU frames the device sees, their CPU coefficients, scan and streams) — made once, then only read."""
    if (name, subsampling) not in _made:
        from pix2pix3d_amd import video
        make, _, quality = CASES[name]
        frames = make()
        if name == 'every second frame':
            frames = frames[::2].contiguous()
        tables = video.jpeg_tables(quality)
        coefficients = video.jpeg_coefficients(frames, tables, subsampling)
        data, offsets = video.jpeg_scan(coefficients, frames.shape[1], frames.shape[2], subsampling)
        header, scans = video.jpeg_header(frames.shape[1], frames.shape[2], tables, subsampling), bytes(data.tolist())
        streams = [header + scans[offsets[i]:offsets[i + 1]] + b'\xff\xd9' for i in range(frames.shape[0])]      # what encode_jpeg assembles
        _made[name, subsampling] = dict(frames=frames, tables=tables, coefficients=coefficients, scan=(data, offsets), streams=streams)
    return _made[name, subsampling]


def _launches(fn, expected):
    from pix2pix3d_amd import video
    n0 = video.launch_count()
    out = fn()
    assert video.launch_count() == n0 + expected, (video.launch_count() - n0, expected)
    return out


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
@pytest.mark.parametrize('name', list(CASES))
def test_the_bytes_equal_the_cpu_formulation(hip_lib, name, subsampling):
    from pix2pix3d_amd import video
    ref = _case(name, subsampling)
    _, put, quality = CASES[name]
    frames = put(CASES[name][0]())
    f, h, w = frames.shape[:3]
    tables = tuple(t.cuda() for t in ref['tables'])
    coefficients = _launches(lambda: video.jpeg_coefficients(frames, tables, subsampling), 1)
    assert coefficients.is_cuda and coefficients.dtype == torch.int16 and torch.equal(coefficients.cpu(), ref['coefficients'])
    data, offsets = _launches(lambda: video.jpeg_scan(coefficients, h, w, subsampling), 2)
    assert data.is_cuda and data.dtype == torch.uint8 and torch.equal(offsets, ref['scan'][1]) and torch.equal(data.cpu(), ref['scan'][0])
    assert _launches(lambda: video.encode_jpeg(frames, quality, subsampling), 3) == ref['streams']
    if name == 'one colour':
        assert not ref['coefficients'][..., 1:].any() and len(set(ref['streams'])) == 1
    if name == 'noise at quality 100':
        assert (ref['scan'][0] == 255).sum() >= 3                                    # stuffing happened
    if name == 'ten intervals a frame':
        assert video.jpeg_layout(h, w, subsampling)[3] > 8


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_the_scan_of_crafted_coefficients(hip_lib, subsampling):
    """Every size category, both signs, runs past 16, 32 and 48 zeros, blocks that end on coefficient 63 — and values past the range, which both clamp."""
    from pix2pix3d_amd import video
    h, w = (24, 200) if subsampling == '4:4:4' else (48, 400)
    _, n_mcu, bpm, _ = video.jpeg_layout(h, w, subsampling)
    coefficients = random_coefficients(3, n_mcu, bpm, seed=62, density=0.5)
    coefficients[0, :, :, 63] = 1
    coefficients[1, 0, 0, :3] = torch.tensor([3000, -3000, 1024], dtype=torch.int16)
    coefficients[2, 1::2] = 0
    want = video.jpeg_scan(coefficients, h, w, subsampling)
    data, offsets = _launches(lambda: video.jpeg_scan(coefficients.cuda(), h, w, subsampling), 2)
    assert torch.equal(offsets, want[1]) and torch.equal(data.cpu(), want[0])


def test_no_frames_launch_nothing(hip_lib):
    from pix2pix3d_amd import video
    frames = torch.empty([0, 16, 16, 3], dtype=torch.uint8, device='cuda')
    tables = tuple(t.cuda() for t in video.jpeg_tables(90))
    coefficients = _launches(lambda: video.jpeg_coefficients(frames, tables), 0)
    assert coefficients.is_cuda and tuple(coefficients.shape) == (0, 0, 6, 64)
    data, offsets = _launches(lambda: video.jpeg_scan(coefficients, 16, 16), 0)
    assert data.is_cuda and data.numel() == 0 and offsets.tolist() == [0]
    assert _launches(lambda: video.encode_jpeg(frames), 0) == []


def test_the_entry_points_refuse_bad_arguments_before_any_launch(hip_lib):
    from pix2pix3d_amd import video, _lib
    frames = noise_frames(1, 8, 8).cuda()
    luma, chroma = (t.cuda() for t in video.jpeg_tables(90))
    out = torch.zeros([1, 1, 3, 64], dtype=torch.int16, device='cuda')
    lengths = torch.zeros([1], dtype=torch.int32, device='cuda')
    huffman = video.jpeg_huffman().lookup.cuda()
    lib, n0 = video.video_lib(), video.launch_count()
    stream = _lib.stream_of(frames)
    blocks = lambda *a: lib.p3d_video_jpeg_blocks(_lib.ptr(frames), *a, _lib.ptr(luma), _lib.ptr(chroma), _lib.ptr(out), stream)
    assert blocks(192, 23, 1, 8, 8, 0) == _lib.P3D_ERR_ARGUMENT                     # a row pitch under 3 w
    assert blocks(192, 24, 1, 8, 8, 2) == _lib.P3D_ERR_ARGUMENT                     # 4:2:2 is not served
    assert blocks(192, 24, -1, 8, 8, 0) == _lib.P3D_ERR_ARGUMENT
    assert blocks(0, 3 << 16, 2, 1 << 15, 1 << 15, 0) == _lib.P3D_ERR_ARGUMENT      # 2^31 pixels
    assert lib.p3d_video_jpeg_blocks(_lib.ptr(frames), 192, 24, 1, 8, 8, 0, None, _lib.ptr(chroma), _lib.ptr(out), stream) == _lib.P3D_ERR_ARGUMENT
    scan = lambda c, sub, lengths, offsets, data, n: lib.p3d_video_jpeg_scan(c, 1, 8, 8, sub, _lib.ptr(huffman), lengths, offsets, data, n, stream)
    assert scan(_lib.ptr(out), 3, _lib.ptr(lengths), None, None, 0) == _lib.P3D_ERR_ARGUMENT
    assert scan(_lib.ptr(out), 0, None, None, None, 0) == _lib.P3D_ERR_ARGUMENT      # the first launch needs lengths
    assert scan(_lib.ptr(out), 0, None, None, _lib.ptr(frames), 192) == _lib.P3D_ERR_ARGUMENT      # the second needs offsets
    assert scan(ctypes.c_void_p(out.data_ptr() + 2), 0, _lib.ptr(lengths), None, None, 0) == _lib.P3D_ERR_ARGUMENT      # 16-byte loads need alignment
    assert scan(_lib.ptr(out), 0, _lib.ptr(lengths), None, None, -1) == _lib.P3D_ERR_ARGUMENT
    assert video.launch_count() == n0 and b'video_jpeg_scan' in lib.p3d_last_error()


def test_one_synchronisation_and_one_copy(hip_lib):
    """torch's sync debug mode reports every synchronising call: ``jpeg_scan`` makes one (the interval lengths), ``encode_jpeg`` that and the copy of the
    scans; ``jpeg_coefficients`` makes none.  The constant tables reach the device on the first call, before the count."""
    from pix2pix3d_amd import video
    frames = gradient_frames(3, 37, 53, seed=63).cuda()
    tables = tuple(t.cuda() for t in video.jpeg_tables(90))
    video.encode_jpeg(frames, 90)
    torch.cuda.synchronize()

    def reported(fn):
        mode = torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            torch.cuda.set_sync_debug_mode('warn')
            try:
                out = fn()
            finally:
                torch.cuda.set_sync_debug_mode(mode)
        return out, [w for w in caught if 'called a synchronizing' in str(w.message)]      # (switching the mode on warns too: a prototype feature)
    coefficients, syncs = reported(lambda: video.jpeg_coefficients(frames, tables))
    assert len(syncs) == 0
    _, syncs = reported(lambda: video.jpeg_scan(coefficients, 37, 53))
    assert len(syncs) == 1, [str(w.message) for w in syncs]
    streams, syncs = reported(lambda: video.encode_jpeg(frames, 90))
    assert len(syncs) == 2, [str(w.message) for w in syncs]
    assert streams == video.encode_jpeg(frames.cpu(), 90)


def test_generate_video_writes_both_avis_from_device_frames(hip_lib, tmp_path):
    from model_cases import build_generator
    from pix2pix3d_amd import views, video
    G = build_generator('seg2cat', 'cuda', depth=(64, 64))
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(41)).cuda()
    n0 = video.launch_count()
    out = views.generate_video(G, ws, 'seg2cat', str(tmp_path / 'v.avi'), str(tmp_path / 'l.avi'), n_frames=4, views_per_step=4, format='avi')
    assert video.launch_count() == n0 + 6 and out['image'].is_cuda                  # three launches a clip
    for path, frames in ((tmp_path / 'v.avi', out['image']), (tmp_path / 'l.avi', out['label'])):
        streams, fps, size = video.read_avi(path)
        assert fps == 60 and size == (frames.shape[2], frames.shape[1]) and streams == video.encode_jpeg(frames.cpu())
