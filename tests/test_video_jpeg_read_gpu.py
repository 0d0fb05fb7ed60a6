"""Reading JPEGs back on the device: p3d_video_jpeg_unscan against the CPU formulation (integer equality of coefficients AND status) on the streams of
test_video_jpeg_read_host.py — our own coder's, Pillow's with optimised tables and its own restart intervals — in batches whose frames differ in their
tables, with more intervals a frame than a wave has lanes; decode_jpeg / decode_avi / check_avi against jpeg_reconstruct; the launches p3d_video.h
states and no synchronisation; and the status of damaged scans.  Small shapes throughout: the subject is the bits, not the throughput."""
import warnings

import numpy as np
import pytest
import torch

import jpeg_read_cases as C
from jpeg_cases import PICTURES
from video_cases import gradient_frames, noise_frames

pytestmark = pytest.mark.gpu


def _launches(fn, expected):
    from pix2pix3d_amd import video
    n0 = video.launch_count()
    out = fn()
    assert video.launch_count() == n0 + expected, (video.launch_count() - n0, expected)
    return out


def _on_device(arguments):
    return tuple(a.cuda() if torch.is_tensor(a) else a for a in arguments)


def _same(arguments):
    """Device ``jpeg_unscan`` of the arguments — a fill and a launch — equals the CPU formulation's: coefficients and status."""
    from pix2pix3d_amd import video
    want, want_status = video.jpeg_unscan(*arguments)
    coefficients, status = _launches(lambda: video.jpeg_unscan(*_on_device(arguments)), 2)
    assert coefficients.is_cuda and status.is_cuda and coefficients.dtype == torch.int16 and status.dtype == torch.int32
    assert torch.equal(status.cpu(), want_status) and torch.equal(coefficients.cpu(), want)
    return want, want_status


@pytest.mark.parametrize('name', list(C.ROUND_TRIPS))
def test_our_own_streams(hip_lib, name):
    from pix2pix3d_amd import video
    c = C.round_trip(name)
    n_intervals = video.jpeg_layout(c['h'], c['w'], c['subsampling'])[3]
    want, status = _same((c['data'], C.own_ranges(c['data'], c['offsets'], n_intervals), c['h'], c['w'], c['subsampling']))
    assert not status.any() and torch.equal(want, c['coefficients'])


@pytest.mark.parametrize('picture', C.FOREIGN_PICTURES)
def test_foreign_streams(hip_lib, picture):
    for label, stream, _ in C.foreign_streams():
        if label.startswith(picture + ' '):
            _, status = _same(C.unscan_arguments(stream))
            assert not status.any(), label


def _batch(streams):
    """The arguments of ONE ``jpeg_unscan`` call over streams of one geometry, each frame with its own table set."""
    from pix2pix3d_amd import video
    infos = [video.jpeg_parse(s) for s in streams]
    first = infos[0]
    assert all((i.h, i.w, i.subsampling, i.components, i.restart) == (first.h, first.w, first.subsampling, first.components, first.restart) for i in infos)
    scans = [s[i.scan[0]:i.scan[1]] for s, i in zip(streams, infos)]
    starts = np.cumsum([0] + [len(s) for s in scans])
    data = torch.tensor(list(b''.join(scans)), dtype=torch.uint8)
    ranges = torch.from_numpy(np.stack([i.intervals - i.scan[0] + starts[k] for k, i in enumerate(infos)]))
    tables = torch.stack([torch.stack([video.jpeg_decode_tables(*t) for t in i.huffman]) for i in infos])
    return (data, ranges, first.h, first.w, first.subsampling, tables, torch.arange(len(infos), dtype=torch.int32), first.restart, first.components), infos


def test_three_frames_with_three_sets_of_optimised_tables(hip_lib):
    streams = [C.pillow_jpeg(PICTURES['gradient'], 'RGB', quality=q, subsampling=2, optimize=True, restart_marker_blocks=2) for q in (50, 75, 90)]
    arguments, infos = _batch(streams)
    assert len({i.huffman for i in infos}) == 3
    want, status = _same(arguments)
    assert not status.any()
    for k, stream in enumerate(streams):
        assert torch.equal(want[k], torch.from_numpy(C.reference_decode(stream)[0]))


def test_81_intervals_a_frame(hip_lib):
    """More than one wave of lanes a frame, and no multiple of 64: the second work-group of every frame is partly idle."""
    pictures = noise_frames(2, 72, 72, seed=81).numpy()
    arguments, infos = _batch([C.pillow_jpeg(p, 'RGB', quality=90, subsampling=0, restart_marker_blocks=1) for p in pictures])
    assert tuple(arguments[1].shape) == (2, 81, 2)
    _, status = _same(arguments)
    assert not status.any()


def test_decode_jpeg_and_the_avi(hip_lib, tmp_path):
    from pix2pix3d_amd import quality, video
    picture = PICTURES['gradient']
    streams = [video.encode_jpeg(torch.from_numpy(picture)[None], 90, '4:2:0')[0], C.pillow_jpeg(picture, 'RGB', quality=50, subsampling=0, optimize=True),
               C.pillow_jpeg(picture, 'L', quality=90, restart_marker_blocks=1), C.pillow_jpeg(picture, 'RGB', quality=90, subsampling=2, restart_marker_rows=1)]
    want = video.decode_jpeg(streams)
    shown = video.decode_jpeg(streams, device='cuda')
    assert shown.is_cuda and torch.equal(shown.cpu(), want)
    clip = torch.cat([gradient_frames(2, 40, 56, seed=82), noise_frames(1, 40, 56, seed=83)]).cuda()
    video.save_avi(tmp_path / 'c.avi', clip, fps=30, quality=90, subsampling='4:2:0')
    frames, fps = video.decode_avi(tmp_path / 'c.avi', device='cuda')
    assert fps == 30 and frames.is_cuda and torch.equal(frames, video.jpeg_reconstruct(clip, 90, '4:2:0'))
    assert torch.equal(frames.cpu(), video.decode_avi(tmp_path / 'c.avi')[0])
    metrics = video.check_avi(tmp_path / 'c.avi', clip, 90, '4:2:0')
    assert metrics['exact'] is True and metrics['psnr'] == quality.compare(video.jpeg_reconstruct(clip, 90, '4:2:0'), clip)['psnr']
    assert video.check_avi(tmp_path / 'c.avi', clip, 75, '4:2:0')['exact'] is False


def test_the_launches_and_no_synchronisation(hip_lib):
    """One fill and one unscan launch a group, two decode launches a run of frames with equal tables; with ``errors='status'`` torch's sync debug mode
    reports nothing, with ``errors='raise'`` the one copy of the status."""
    from pix2pix3d_amd import video
    x = gradient_frames(4, 40, 56, seed=84)
    streams = video.encode_jpeg(x[:2], 90) + video.encode_jpeg(x[2:], 50)             # one group, two runs of tables
    foreign = [C.pillow_jpeg(x[0].numpy(), 'RGB', quality=90, subsampling=0, restart_marker_blocks=2)]      # a second group
    video.decode_jpeg(streams + foreign, device='cuda')
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
        return out, [w for w in caught if 'called a synchronizing' in str(w.message)]
    (frames, status), syncs = reported(lambda: _launches(lambda: video.decode_jpeg(streams, device='cuda', errors='status'), 2 + 2 * 2))
    assert len(syncs) == 0, [str(w.message) for w in syncs]
    assert not status.any() and torch.equal(frames.cpu(), torch.cat([video.jpeg_reconstruct(x[:2], 90), video.jpeg_reconstruct(x[2:], 50)]))
    (frames, status), syncs = reported(lambda: _launches(lambda: video.decode_jpeg(streams + foreign, device='cuda', errors='status'), 2 * 2 + 2 * 3))
    assert len(syncs) == 0, [str(w.message) for w in syncs]
    _, syncs = reported(lambda: _launches(lambda: video.decode_jpeg(streams, device='cuda'), 2 + 2 * 2))
    assert len(syncs) == 1, [str(w.message) for w in syncs]


def test_damaged_scans_on_the_device(hip_lib, tmp_path):
    """The status of the damaged inputs — jpeg_read_cases.damaged_streams(), the list the stand-alone program of test_video_jpeg_read_host.py runs under the
    sanitizers — equals the CPU formulation's.  The same program, as a plain host build, goes over them here first: no input reaches the device that the
    routine has not already taken on the host.  The subject is the flags; safety is the routine's clamps."""
    from pix2pix3d_amd import video
    cases = [(label, C.unscan_arguments(stream)) for label, stream, _ in C.damaged_streams()]
    exe, _ = C.build_checker(str(tmp_path), sanitize=False)
    on_host = C.run_checker(exe, cases, str(tmp_path))
    for (label, arguments), (_, host_status) in zip(cases, on_host):
        want, want_status = video.jpeg_unscan(*arguments)
        assert want_status.any() and torch.equal(host_status, want_status), label
        coefficients, status = video.jpeg_unscan(*_on_device(arguments))
        assert torch.equal(status.cpu(), want_status) and torch.equal(coefficients.cpu(), want), label
    stream = C.damaged_streams()[0][1]
    with pytest.raises(ValueError, match='does not decode'):
        video.decode_jpeg([stream], device='cuda')


def test_the_entry_point_refuses_bad_arguments_before_any_launch(hip_lib):
    from pix2pix3d_amd import video, _lib
    data, ranges, h, w, subsampling, tables, table_of_frame, restart, components = _on_device(C.unscan_arguments(C.foreign_streams()[0][1]))
    out = torch.zeros([1, video.jpeg_layout(h, w, subsampling)[1], 3, 64], dtype=torch.int16, device='cuda')
    status = torch.zeros([1, 1], dtype=torch.int32, device='cuda')
    lib, n0 = video.video_lib(), video.launch_count()
    stream = _lib.stream_of(out)

    def call(data_bytes=data.shape[0], n_sets=1, f=1, h=h, w=w, sub=0, components=3, restart=1, ranges=ranges, out=out):
        return lib.p3d_video_jpeg_unscan(_lib.ptr(data), data_bytes, _lib.ptr(ranges), _lib.ptr(tables), n_sets, _lib.ptr(table_of_frame), f, h, w, sub,
                                         components, restart, _lib.ptr(out), _lib.ptr(status), stream)
    for bad in (dict(data_bytes=-1), dict(n_sets=0), dict(f=-1), dict(sub=2), dict(components=2), dict(components=1, sub=1), dict(restart=0),
                dict(ranges=None), dict(out=None), dict(h=1 << 16, w=1 << 16)):
        assert call(**bad) == _lib.P3D_ERR_ARGUMENT, bad
    assert video.launch_count() == n0 and b'video_jpeg_unscan' in lib.p3d_last_error()
    assert call(f=0) == _lib.P3D_OK and video.launch_count() == n0                  # no frame: nothing to do
