"""pix2pix3d_amd.video's PNG kernels on the device: the bytes of p3d_video_png_filter, p3d_video_png_count and p3d_video_png_emit against the CPU formulation
(integer equality) and the launch counts p3d_video.h states, at the smallest shapes that can go wrong: a pitched, offset window of a canvas; a strided selection
of frames; 1 .. 4 bytes a pixel on rows that are no multiple of 4; one pixel; one colour (runs far beyond 258 that cross every step of the walk and end with
their segment); every way a run can end; runs around the walk's 64-byte steps; noise (no match, the flattest code); a histogram that needs the 15-bit limit;
one row a segment and a shorter last segment; a segment per frame over many frames; no frame at all."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from png_cases import chunk_straddlers, crafted_rows, decode_apng, fibonacci_frame, mode_frames
from video_cases import gradient_frames, noise_frames

pytestmark = pytest.mark.gpu


def _window(frames):
    """The frames as an offset, pitched window of a larger device canvas of other bytes."""
    f, h, w = frames.shape[:3]
    canvas = torch.from_numpy(np.random.default_rng(81).integers(0, 256, size=(f + 1, h + 5, w + 7) + tuple(frames.shape[3:]), dtype=np.uint8)).cuda()
    view = canvas[1:, 2:2 + h, 3:3 + w]
    view.copy_(frames)
    assert not view.is_contiguous() and view.data_ptr() != canvas.data_ptr()
    return view


def _w37(bpp):
    frames = torch.from_numpy(np.random.default_rng(82 + bpp).integers(0, 256, size=[2, 9, 37, bpp], dtype=np.uint8) // 64 * 60)      # four values: short runs
    frames[1, 3:6] = frames[1, 2:3]                                                # rows that repeat: Up
    return frames[..., 0] if bpp == 1 else frames


def _single_colour(colour):
    frames = torch.empty([2, 128, 160, 3], dtype=torch.uint8)
    frames[:] = torch.tensor(colour, dtype=torch.uint8)
    return frames


_up = lambda t: t.cuda()
CASES = {
    # name: (CPU frames, how they reach the device, filter, segment_rows or None for the module's rule)
    'a window of a canvas': (lambda: torch.cat([gradient_frames(2, 37, 53, seed=83), noise_frames(1, 37, 53, seed=84)]), _window, 5, None),
    'every second frame': (lambda: gradient_frames(5, 37, 53, seed=85), lambda t: t.cuda()[::2], 5, 8),
    'one byte a pixel, rows of 38': (lambda: _w37(1), _up, 5, 4),
    'two bytes a pixel, rows of 75': (lambda: _w37(2), _up, 5, 4),
    'three bytes a pixel, rows of 112': (lambda: _w37(3), _up, 5, 4),
    'four bytes a pixel, rows of 149': (lambda: _w37(4), _up, 5, 4),
    'four bytes a pixel in a window': (lambda: mode_frames('RGBA')[0], _window, 4, 5),
    'one pixel': (lambda: noise_frames(1, 1, 1, seed=86), _up, 5, None),
    'one colour': (lambda: _single_colour([0, 0, 0]), _up, 0, None),              # 68 rows a segment, the type bytes zeros too: ONE run of 32708 bytes, ending with its segment
    'one colour, filtered': (lambda: _single_colour([201, 17, 94]), _up, 5, None),      # Up: a run of 480 zeros after every type byte
    'every way a run can end': (crafted_rows, _up, 0, 1),
    'runs around the steps of the walk': (chunk_straddlers, _up, 0, 1),
    'noise, unfiltered': (lambda: noise_frames(2, 24, 40, seed=87), _up, 0, None),
    'a histogram that needs the limit': (fibonacci_frame, _up, 0, None),
    'a row a segment': (lambda: gradient_frames(1, 70, 19, seed=88), _up, 5, 1),
    'a shorter last segment': (lambda: gradient_frames(2, 10, 19, seed=89), _up, 5, 4),
    'a segment per frame': (lambda: noise_frames(600, 8, 8, seed=90) // 32 * 32, _up, 5, None),
}
_made = {}


def _case(name):
    """(the CPU frames the device sees, their filtered rows, counts, streams and files by the CPU formulation) — made once, then only read."""
    if name not in _made:
        from pix2pix3d_amd import video
        make, _, filt, rows = CASES[name]
        frames = make()
        if name == 'every second frame':
            frames = frames[::2].contiguous()
        bpp = frames.shape[3] if frames.ndim == 4 else 1
        rows = video.png_segment_rows(frames.shape[2], bpp) if rows is None else rows
        filtered = video.png_filter(frames, filt)
        _made[name] = dict(frames=frames, rows=rows, filtered=filtered, stats=video.png_counts(filtered, rows), deflate=video.png_deflate(filtered, rows),
                           files=video.encode_png(frames, filter=filt))
    return _made[name]


def _launches(fn, expected):
    from pix2pix3d_amd import video
    n0 = video.launch_count()
    out = fn()
    assert video.launch_count() == n0 + expected, (video.launch_count() - n0, expected)
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_the_bytes_equal_the_cpu_formulation(hip_lib, name):
    from pix2pix3d_amd import video
    ref = _case(name)
    make, put, filt, _ = CASES[name]
    frames = put(make())
    assert tuple(frames.shape) == tuple(ref['frames'].shape)
    filtered = _launches(lambda: video.png_filter(frames, filt), 1)
    assert filtered.is_cuda and filtered.dtype == torch.uint8 and torch.equal(filtered.cpu(), ref['filtered'])
    stats = _launches(lambda: video.png_counts(filtered, ref['rows']), 1)
    assert stats.is_cuda and stats.dtype == torch.int32 and torch.equal(stats.cpu(), ref['stats'])
    data, offsets = _launches(lambda: video.png_deflate(filtered, ref['rows']), 2)      # the counts again, then the bytes
    assert data.is_cuda and data.dtype == torch.uint8 and torch.equal(offsets, ref['deflate'][1]) and torch.equal(data.cpu(), ref['deflate'][0])
    assert _launches(lambda: video.encode_png(frames, filter=filt), 3) == ref['files']
    if name == 'one colour':
        assert ref['stats'].shape[1] == 2 and ref['stats'][0, 0, [0, 285, 287]].tolist() == [1, 126, 127]      # 32707 = 126 * 258 + 199
    if name == 'noise, unfiltered':
        assert int(ref['stats'][..., 287].sum()) <= 2                                    # (next to) no match
    if name == 'a histogram that needs the limit':
        counts = ref['stats'][0, :, :286].sum(dim=0)
        counts[256] = ref['stats'].shape[1]
        assert video.png_code_lengths(counts)[1] == 15 and ref['stats'].shape[1] > 30
    if name == 'a row a segment':
        assert ref['stats'].shape[1] == 70
    if name == 'a segment per frame':
        assert tuple(ref['stats'].shape[:2]) == (600, 1)


def test_indices_with_a_palette_and_sixteen_bits(hip_lib):
    from pix2pix3d_amd import video
    indices, palette = mode_frames('P')
    assert _launches(lambda: video.encode_png(indices.cuda(), 'P', palette.cuda()), 3) == video.encode_png(indices, 'P', palette)
    depth = torch.linspace(0.2, 4.0, 2 * 13 * 37, dtype=torch.float32).reshape(2, 13, 37).cuda()
    pairs = video.depth16(depth, 0.5, 3.5)
    assert pairs.is_cuda and torch.equal(pairs.cpu(), video.depth16(depth.cpu(), 0.5, 3.5))
    assert video.encode_png(pairs, 'I;16') == video.encode_png(pairs.cpu(), 'I;16')


def test_the_apng_from_device_frames_is_the_hosts(hip_lib, tmp_path):
    from pix2pix3d_amd import video
    frames = torch.cat([gradient_frames(3, 37, 53, seed=91), noise_frames(1, 37, 53, seed=92)])
    streams = _launches(lambda: video.save_apng(tmp_path / 'device.png', frames.cuda(), fps=50), 3)
    assert streams == video.save_apng(tmp_path / 'host.png', frames, fps=50)
    assert (tmp_path / 'device.png').read_bytes() == (tmp_path / 'host.png').read_bytes()
    got, durations, _ = decode_apng(tmp_path / 'device.png')
    assert all(np.array_equal(g, f.numpy()) for g, f in zip(got, frames)) and durations == [20.0] * 4
    paths = _launches(lambda: video.save_png_sequence(str(tmp_path / 's{}.png'), frames.cuda()), 3)
    assert [open(p, 'rb').read() for p in paths] == video.encode_png(frames)


def test_no_frames_and_no_pixels_launch_nothing(hip_lib):
    from pix2pix3d_amd import video
    for shape in ([0, 16, 16, 3], [2, 0, 16, 3], [2, 16, 0, 3], [0, 16, 16]):
        frames = torch.empty(shape, dtype=torch.uint8, device='cuda')
        filtered = _launches(lambda: video.png_filter(frames), 0)
        bpp = shape[3] if len(shape) == 4 else 1
        assert filtered.is_cuda and tuple(filtered.shape) == (shape[0], shape[1], 1 + shape[2] * bpp)
        stats = _launches(lambda: video.png_counts(filtered, 4), 0)
        assert stats.is_cuda and stats.shape[0] == shape[0] and not stats.any()
        data, offsets = _launches(lambda: video.png_deflate(filtered, 4), 0)
        assert data.is_cuda and data.numel() == 0 and offsets.tolist() == [0] * (shape[0] + 1)
    assert _launches(lambda: video.encode_png(torch.empty([0, 16, 16, 3], dtype=torch.uint8, device='cuda')), 0) == []


def test_the_entry_points_refuse_bad_arguments_before_any_launch(hip_lib):
    from pix2pix3d_amd import video, _lib
    frames = noise_frames(1, 8, 8).cuda()
    filtered = torch.zeros([1, 8, 25], dtype=torch.uint8, device='cuda')
    stats = torch.zeros([1, 2, video.PNG_STATS], dtype=torch.int32, device='cuda')
    words = torch.zeros([1024], dtype=torch.int32, device='cuda')
    offsets = torch.zeros([2], dtype=torch.int64, device='cuda')
    data = torch.zeros([4096], dtype=torch.uint8, device='cuda')
    lib, n0 = video.video_lib(), video.launch_count()
    stream = _lib.stream_of(frames)
    P = _lib.ptr
    flt = lambda pitch, f, h, w, bpp, filt, src=P(frames), dst=P(filtered): lib.p3d_video_png_filter(src, 192, pitch, f, h, w, bpp, filt, dst, stream)
    assert flt(23, 1, 8, 8, 3, 5) == _lib.P3D_ERR_ARGUMENT                          # a row pitch under w bpp
    assert flt(24, 1, 8, 8, 0, 5) == _lib.P3D_ERR_ARGUMENT and flt(24, 1, 8, 8, 5, 5) == _lib.P3D_ERR_ARGUMENT
    assert flt(24, 1, 8, 8, 3, 6) == _lib.P3D_ERR_ARGUMENT and flt(24, 1, 8, 8, 3, -1) == _lib.P3D_ERR_ARGUMENT
    assert flt(24, -1, 8, 8, 3, 5) == _lib.P3D_ERR_ARGUMENT
    assert flt(1 << 20, 2, 1 << 15, 1 << 13, 4, 5) == _lib.P3D_ERR_ARGUMENT          # 2^31 bytes
    assert flt(1 << 20, 1, 1 << 16, (1 << 15) - 1, 1, 5) == _lib.P3D_ERR_ARGUMENT    # 2^31 filtered bytes: the type bytes count
    assert flt(24, 1, 8, 8, 3, 5, src=None) == _lib.P3D_ERR_ARGUMENT and flt(24, 1, 8, 8, 3, 5, dst=None) == _lib.P3D_ERR_ARGUMENT
    assert b'video_png_filter' in lib.p3d_last_error()
    cnt = lambda f, h, r, rows, src=P(filtered), dst=P(stats): lib.p3d_video_png_count(src, f, h, r, rows, dst, stream)
    assert cnt(1, 8, 25, 0) == _lib.P3D_ERR_ARGUMENT and cnt(1, 8, -25, 4) == _lib.P3D_ERR_ARGUMENT
    assert cnt(1 << 11, 1 << 10, 1 << 10, 4) == _lib.P3D_ERR_ARGUMENT
    assert cnt(1, 8, 25, 4, src=None) == _lib.P3D_ERR_ARGUMENT and cnt(1, 8, 25, 4, dst=None) == _lib.P3D_ERR_ARGUMENT
    assert cnt(1, 8, 25, 4, dst=ctypes.c_void_p(stats.data_ptr() + 2)) == _lib.P3D_ERR_ARGUMENT
    assert b'video_png_count' in lib.p3d_last_error()

    def emit(rows=4, n=4096, src=P(filtered), tables=P(words), headers=P(words), bits=P(words), adler=P(words), at=P(offsets), dst=P(data)):
        return lib.p3d_video_png_emit(src, 1, 8, 25, rows, tables, headers, bits, adler, at, dst, n, stream)
    assert emit(rows=0) == _lib.P3D_ERR_ARGUMENT and emit(n=-1) == _lib.P3D_ERR_ARGUMENT
    for name in ('src', 'tables', 'headers', 'bits', 'adler', 'at', 'dst'):
        assert emit(**{name: None}) == _lib.P3D_ERR_ARGUMENT, name
    assert emit(at=ctypes.c_void_p(offsets.data_ptr() + 4)) == _lib.P3D_ERR_ARGUMENT and emit(tables=ctypes.c_void_p(words.data_ptr() + 2)) == _lib.P3D_ERR_ARGUMENT
    assert video.launch_count() == n0 and b'video_png_emit' in lib.p3d_last_error()


def test_one_synchronisation_and_one_copy(hip_lib):
    """torch's sync debug mode reports every synchronising call: ``png_filter`` and ``png_counts`` make none, ``png_deflate`` one (the counts come to the host;
    what goes up leaves pinned memory without a wait), ``encode_png`` that and the copy of the bytes."""
    from pix2pix3d_amd import video
    frames = gradient_frames(3, 37, 53, seed=93).cuda()
    video.encode_png(frames)
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
    filtered, syncs = reported(lambda: video.png_filter(frames))
    assert len(syncs) == 0
    _, syncs = reported(lambda: video.png_counts(filtered, 8))
    assert len(syncs) == 0
    _, syncs = reported(lambda: video.png_deflate(filtered, 8))
    assert len(syncs) == 1, [str(w.message) for w in syncs]
    files, syncs = reported(lambda: video.encode_png(frames))
    assert len(syncs) == 2, [str(w.message) for w in syncs]
    assert files == video.encode_png(frames.cpu())


def test_generate_video_and_generate_sample_write_lossless_files_from_device_frames(hip_lib, tmp_path):
    from PIL import Image
    from model_cases import build_generator
    from pix2pix3d_amd import views, video
    G = build_generator('seg2cat', 'cuda', depth=(64, 64))
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(41)).cuda()
    n0 = video.launch_count()
    out = views.generate_video(G, ws, 'seg2cat', str(tmp_path / 'v.png'), str(tmp_path / 'l.png'), n_frames=4, views_per_step=4, format='apng')
    assert video.launch_count() == n0 + 6 and out['image'].is_cuda                  # three launches a clip
    got, _, _ = decode_apng(tmp_path / 'v.png')
    assert all(np.array_equal(g, f.cpu().numpy()) for g, f in zip(got, out['image']))
    with Image.open(tmp_path / 'l.png') as im:
        assert im.mode == 'P' and im.n_frames == 4
        for i in range(4):
            im.seek(i)
            assert np.array_equal(np.asarray(im), out['label_index'][i].cpu().numpy())
            assert np.array_equal(np.asarray(im.convert('RGB')), out['label'][i].cpu().numpy())
    sample = views.generate_sample(G, ws, views.video_cameras(G, 'seg2cat', 4)[0], str(tmp_path / 'c.png'), str(tmp_path / 's.png'), png='device')
    assert video.launch_count() == n0 + 12
    with Image.open(tmp_path / 'c.png') as c, Image.open(tmp_path / 's.png') as s:
        assert np.array_equal(np.asarray(c), sample['image'][0].cpu().numpy()) and np.array_equal(np.asarray(s.convert('RGB')), sample['label'][0].cpu().numpy())
