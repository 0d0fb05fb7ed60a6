"""Reading PNG and APNG back on the device: p3d_video_png_inflate and p3d_video_png_unfilter against the CPU formulations (integer equality of bytes AND
status) on the inputs of test_video_png_read_host.py — our own writer's streams with and without the segment index, Pillow's, raw zlib's — in batches
whose frames are different streams of different lengths and with more parts than a work-group has lanes; the un-filter at the shapes where its
wavefront can go wrong; decode_png / decode_apng / check_png on device frames; the launches p3d_video.h states and no synchronisation; the status of
damaged inputs; and the argument checks.  Small shapes throughout: the subject is the bits, not the throughput."""
import warnings

import numpy as np
import pytest
import torch

import png_cases
import png_read_cases as C

pytestmark = pytest.mark.gpu
DEFINITION_BYTES = 300_000      # above it (the Fibonacci frame) the device is held against zlib's bytes, which the host tests show to be the definition's


def _launches(fn, expected):
    from pix2pix3d_amd import video
    n0 = video.launch_count()
    out = fn()
    assert video.launch_count() == n0 + expected, (video.launch_count() - n0, expected)
    return out


def _same_inflate(label, data, parts, out_bytes, want=None):
    """Device ``png_inflate`` — a fill and a launch — equals the CPU formulation's bytes and status (or zlib's bytes with a clean status)."""
    from pix2pix3d_amd import video
    out, status = _launches(lambda: video.png_inflate(data.cuda(), parts.cuda(), out_bytes), 2)
    assert out.is_cuda and status.is_cuda and out.dtype == torch.uint8 and status.dtype == torch.int32 and tuple(status.shape) == (parts.shape[0],)
    if want is not None and out_bytes > DEFINITION_BYTES:
        assert not status.any() and bytes(out.cpu().numpy()) == want, label
        return status.cpu()
    definition, definition_status = video.png_inflate(data, parts, out_bytes)
    assert torch.equal(status.cpu(), definition_status) and torch.equal(out.cpu(), definition), (label, status.tolist(), definition_status.tolist())
    return definition_status


@pytest.mark.parametrize('kind', ['own', 'Pillow', 'zlib'])
def test_inflate_on_every_clean_input(hip_lib, kind):
    """... among them more parts (71) than a work-group has lanes (32) and no multiple of them, and the far-match and the two-stored-block streams as
    single parts."""
    from pix2pix3d_amd import video
    seen = 0
    for label, data, parts, out_bytes, want in C.clean_cases():
        if label.startswith(kind + ' '):
            status = _same_inflate(label, data, parts, out_bytes, want)
            assert not status.any(), label
            seen += 1
            if label == 'own fibonacci index=True frame 0':
                assert parts.shape[0] == 71 > video.PNG_INFLATE_LANES and parts.shape[0] % video.PNG_INFLATE_LANES
            if label in ('zlib far match', 'zlib two stored blocks'):
                assert parts.shape[0] == 1
    assert seen >= 5


def test_a_batch_of_different_streams_of_different_lengths(hip_lib):
    """One call over every clean case below 100 KB: the streams joined, the parts shifted to where each went — 40 streams, 49 parts."""
    cases = [c for c in C.clean_cases() if c[3] <= 100_000]
    data = torch.cat([c[1] for c in cases])
    at_in = np.cumsum([0] + [c[1].shape[0] for c in cases])
    at_out = np.cumsum([0] + [c[3] for c in cases])
    parts = torch.cat([c[2] + torch.tensor([at_in[k], at_in[k], at_out[k], at_out[k], 0]) for k, c in enumerate(cases)])
    assert parts.shape[0] > 32 and parts.shape[0] % 32 and len({c[1].shape[0] for c in cases}) > 20
    status = _same_inflate('batch', data, parts, int(at_out[-1]))
    assert not status.any()
    from pix2pix3d_amd import video
    out, _ = video.png_inflate(data.cuda(), parts.cuda(), int(at_out[-1]))
    assert bytes(out.cpu().numpy()) == b''.join(c[4] for c in cases)


UNFILTER_SHAPES = [
    # (F, h, w, bpp): the band edges, one column, rows of 63 / 64 / 65 bytes, every bpp, three frames
    (1, 1, 9, 3), (1, 63, 5, 1), (1, 64, 5, 2), (1, 65, 5, 4), (1, 130, 3, 3), (2, 70, 1, 1), (1, 5, 1, 8), (1, 9, 63, 1), (1, 9, 64, 1), (1, 9, 65, 1), (1, 9, 21, 3),
    (1, 9, 16, 4), (1, 9, 13, 6), (1, 67, 8, 8), (3, 66, 7, 3), (3, 5, 6, 2),
]


@pytest.mark.parametrize('shape', UNFILTER_SHAPES)
def test_unfilter_shapes(hip_lib, shape):
    from pix2pix3d_amd import video
    f, h, w, bpp = shape
    for kind in (0, 1, 2, 3, 4, 'mix'):
        rows = C.filtered_rows(f, h, w, bpp, kind, seed=100 + h + w + bpp)
        want, want_status = video.png_unfilter(rows, bpp)
        shown, status = _launches(lambda: video.png_unfilter(rows.cuda(), bpp), 1)
        assert shown.is_cuda and status.dtype == torch.int32 and tuple(shown.shape) == tuple(want.shape)
        assert torch.equal(status.cpu(), want_status) and not want_status.any() and torch.equal(shown.cpu(), want), (shape, kind)


def test_unfilter_into_a_window_and_with_a_bad_type(hip_lib):
    from pix2pix3d_amd import video
    rows = C.filtered_rows(3, 70, 11, 3, 'mix', seed=120)
    rows[1, 66, 0] = 7
    want, want_status = video.png_unfilter(rows, 3)
    assert want_status.tolist() == [0, C.FILTER, 0]
    canvas = torch.full([3, 80, 20, 3], 99, dtype=torch.uint8, device='cuda')
    window = canvas[:, 4:74, 5:16]
    shown, status = _launches(lambda: video.png_unfilter(rows.cuda(), 3, out=window), 1)
    assert shown.data_ptr() == window.data_ptr() and torch.equal(status.cpu(), want_status) and torch.equal(window.cpu(), want)
    outside = canvas.clone()
    outside[:, 4:74, 5:16] = 99
    assert (outside == 99).all()                                                    # the bytes between rows stay untouched
    x = torch.from_numpy(np.random.default_rng(121).integers(0, 256, size=[2, 130, 67, 4], dtype=np.uint8)).cuda()
    assert torch.equal(video.png_unfilter(video.png_filter(x), 4)[0], x)             # the inverse of the device filter, adaptive types


def _reported(fn):
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    return out, [w for w in caught if 'called a synchronizing' in str(w.message)]


def test_decode_png_the_launches_and_no_synchronisation(hip_lib):
    """Own files of every mode, from device frames and back onto the device; Pillow's; and the launches: a fill and an inflate, an un-filter, the counts
    of the Adler check.  ``errors='status'`` shows no synchronisation under torch's sync debug mode, ``errors='raise'`` the one copy of the status."""
    from pix2pix3d_amd import video
    for label, mode, frames, palette, index, streams in C.own_files():
        shown = video.decode_png(streams, device='cuda')
        assert shown.is_cuda and torch.equal(shown.cpu(), frames), label
        assert video.check_png(streams, frames.cuda()) and (label.startswith('fibonacci') or not video.check_png(streams, frames.cuda().flip(2)))
    for label, stream in C.pillow_files().items():
        assert np.array_equal(video.decode_png([stream], device='cuda')[0].cpu().numpy(), C.pillow_pixels(stream)), label
    frames, _ = png_cases.mode_frames('RGB', f=3)
    streams = video.encode_png(frames.cuda(), index=True)
    assert streams == video.encode_png(frames, index=True)
    torch.cuda.synchronize()
    (shown, status), syncs = _reported(lambda: _launches(lambda: video.decode_png(streams, device='cuda', errors='status'), 2 + 1 + 1))
    assert len(syncs) == 0, [str(w.message) for w in syncs]
    assert status.is_cuda and not status.any() and torch.equal(shown.cpu(), frames)
    (shown, status), syncs = _reported(lambda: _launches(lambda: video.decode_png(streams, device='cuda', errors='status', verify=False), 2 + 1))
    assert len(syncs) == 0 and torch.equal(shown.cpu(), frames)
    shown, syncs = _reported(lambda: _launches(lambda: video.decode_png(streams, device='cuda'), 2 + 1 + 1))
    assert len(syncs) == 1, [str(w.message) for w in syncs]


def test_label_index_frames_depth16_and_the_apng(hip_lib, tmp_path):
    """What the lossless claim is about: palette-index frames as ``views`` writes its label maps and 16-bit depth, checked where they are."""
    from pix2pix3d_amd import edit, video
    rng = np.random.default_rng(130)
    labels = torch.from_numpy((rng.integers(0, 19, size=[4, 1, 1]) + np.arange(70)[None, :, None] // 9 + np.arange(90)[None, None, :] // 11).astype(np.uint8) % 19).cuda()
    palette = torch.from_numpy(rng.integers(0, 256, size=[19, 3], dtype=np.uint8))
    for index in (False, True):
        video.save_apng(tmp_path / 'labels.png', labels, fps=12, mode='P', palette=palette, index=index)
        shown, fps = video.decode_apng(tmp_path / 'labels.png', device='cuda')
        assert fps == 12 and shown.is_cuda and torch.equal(shown, labels) and video.check_png(tmp_path / 'labels.png', labels)
        assert not video.check_png(tmp_path / 'labels.png', labels.roll(1, 0))
    info = video.png_parse((tmp_path / 'labels.png').read_bytes())
    assert torch.equal(video.png_rgb(shown, info), palette.cuda()[labels.long()])
    depth = torch.from_numpy(rng.random([2, 45, 300])).cuda() * 3 + 1
    pairs = video.depth16(depth, 1.0, 4.0)
    streams = video.encode_png(pairs, mode='I;16', index=True)
    assert video.check_png(streams, pairs) and torch.equal(video.decode_png(streams, device='cuda', index=False), pairs)
    video.save_png(tmp_path / 'mask.png', labels[0])
    assert torch.equal(edit.load_mask(tmp_path / 'mask.png', 'cuda'), labels[0])


def test_damaged_inputs_on_the_device(hip_lib, tmp_path):
    """The status of the damaged inputs — png_read_cases.damaged_cases(), the list the stand-alone program of test_video_png_read_host.py runs under the
    sanitizers — equals the CPU formulation's.  The same program, as a plain host build, goes over them here first: no input reaches the device that the
    routine has not already taken on the host.  The subject is the flags; safety is the routine's clamps."""
    from pix2pix3d_amd import video
    cases = C.damaged_cases()
    files = []
    for label, stream, bits in C.damaged_files():                                    # the files' inflate inputs too: lying indices are parts like any other
        info = video.png_parse(stream)
        rows, firsts = info.index[0] if info.index[0] is not None else (info.h, ())
        files.append(C.case_of(label, info.streams[0], firsts, rows * (1 + info.w * video.PNG_MODES[info.mode][0])))
    exe, _ = C.build_checker(str(tmp_path), sanitize=False)
    on_host = C.run_checker(exe, cases + files, str(tmp_path))
    for (label, data, parts, out_bytes, _), (host_out, host_status) in zip(cases + files, on_host):
        want, want_status = video.png_inflate(data, parts, out_bytes)
        assert torch.equal(host_status, want_status) and torch.equal(host_out, want), label
        out, status = video.png_inflate(data.cuda(), parts.cuda(), out_bytes)
        assert torch.equal(status.cpu(), want_status) and torch.equal(out.cpu(), want), label
    assert all(torch.tensor(c[4]).any() for c in cases)
    for label, stream, bits in C.damaged_files():
        want, want_status = video.decode_png([stream], errors='status')
        shown, status = video.decode_png([stream], device='cuda', errors='status')
        assert want_status.any() and torch.equal(status.cpu(), want_status) and torch.equal(shown.cpu(), want), label
        with pytest.raises(ValueError, match='does not decode'):
            video.decode_png([stream], device='cuda')


def test_the_entry_points_refuse_bad_arguments_before_any_launch(hip_lib):
    from pix2pix3d_amd import video, _lib
    _, data, parts, out_bytes, _ = C.clean_cases()[0]
    data, parts = data.cuda(), parts.cuda()
    out = torch.zeros([out_bytes], dtype=torch.uint8, device='cuda')
    status = torch.zeros([4], dtype=torch.int32, device='cuda')
    lib, n0 = video.video_lib(), video.launch_count()
    stream = _lib.stream_of(out)

    def inflate(data=data, data_bytes=data.shape[0], parts=parts, n_parts=1, out=out, out_bytes=out_bytes, status=status):
        return lib.p3d_video_png_inflate(_lib.ptr(data), data_bytes, _lib.ptr(parts), n_parts, _lib.ptr(out), out_bytes, _lib.ptr(status), stream)
    for bad in (dict(data_bytes=-1), dict(out_bytes=-1), dict(n_parts=-1), dict(data=None), dict(parts=None), dict(out=None), dict(status=None)):
        assert inflate(**bad) == _lib.P3D_ERR_ARGUMENT, bad
    assert video.launch_count() == n0 and b'video_png_inflate' in lib.p3d_last_error()
    assert inflate(n_parts=0) == _lib.P3D_OK and video.launch_count() == n0          # no part: nothing to do

    rows = C.filtered_rows(1, 4, 5, 3, 'mix', seed=140).cuda()
    frames = torch.zeros([1, 4, 5, 3], dtype=torch.uint8, device='cuda')

    def unfilter(rows=rows, f=1, h=4, w=5, bpp=3, frames=frames, frame_pitch=60, row_pitch=15, status=status):
        return lib.p3d_video_png_unfilter(_lib.ptr(rows), f, h, w, bpp, _lib.ptr(frames), frame_pitch, row_pitch, _lib.ptr(status), stream)
    for bad in (dict(f=-1), dict(h=-1), dict(w=-1), dict(bpp=0), dict(bpp=9), dict(rows=None), dict(frames=None), dict(status=None), dict(row_pitch=14),
                dict(frame_pitch=-1), dict(h=1 << 16, w=1 << 15), dict(f=1 << 12, h=1 << 10, w=1 << 9)):
        assert unfilter(**bad) == _lib.P3D_ERR_ARGUMENT, bad
    assert video.launch_count() == n0 and b'video_png_unfilter' in lib.p3d_last_error()
    for empty in (dict(f=0), dict(h=0), dict(w=0)):
        assert unfilter(**empty) == _lib.P3D_OK and video.launch_count() == n0      # an empty clip: nothing to do
    assert tuple(video.png_unfilter(torch.zeros([0, 4, 16], dtype=torch.uint8, device='cuda'), 3)[0].shape) == (0, 4, 5, 3) and video.launch_count() == n0
