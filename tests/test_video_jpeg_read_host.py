"""Reading JPEGs back (pix2pix3d_amd.video: jpeg_parse, jpeg_unscan, decode_jpeg, decode_avi, check_avi) on the host: the CPU formulation of the entropy
decoder against a first-principles decoder (jpeg_read_cases.reference_decode: a loop, one bit at a time), bit for bit — on our own coder's streams, on
Pillow's with optimised tables and its own restart intervals, and on damaged scans, where the status bits are part of the contract; the parser's fields
and refusals; the pixels against ``jpeg_reconstruct`` (exactly) and against libjpeg's decoder (a few grey levels); and the routine the device runs, built
for the host under the address and undefined-behaviour sanitizers and run as a program of its own on every input above.  No GPU."""
import io

import numpy as np
import pytest
import torch

import jpeg_read_cases as C
from conftest import record_error
from jpeg_cases import PICTURES, SUBSAMPLINGS, decode, psnr, reference_scan, split_jpeg

# Measured with this case list (40 Pillow streams): the largest difference between jpeg_decode's pixels and libjpeg's is 3 grey levels, the lowest PSNR
# between the two decodes 56.4 dB — the inverse DCTs and the chroma filters round differently.  The bound is the measured maximum plus one level.
PIL_LEVELS = 3 + 1


def _video():
    from pix2pix3d_amd import video
    return video


_decoded = {}


def _foreign(i):
    """(JpegInfo, coefficients, status) of foreign stream i through jpeg_parse and the CPU formulation of jpeg_unscan — made once."""
    if i not in _decoded:
        video = _video()
        stream = C.foreign_streams()[i][1]
        coefficients, status = video.jpeg_unscan(*C.unscan_arguments(stream))
        _decoded[i] = (video.jpeg_parse(stream), coefficients, status)
    return _decoded[i]


def _ac_code_lengths(coefficients):
    """The lengths of the AC Huffman codes that jpeg_scan emits for int16 [..., bpm, 64] coefficients under the Annex K tables: a plain loop."""
    video = _video()
    lookup = video.jpeg_huffman().lookup.numpy().view(np.uint32) >> 16
    bpm, lengths = coefficients.shape[-2], set()
    for j, block in enumerate(coefficients.reshape(-1, 64).tolist()):
        k = j % bpm
        table = lookup[3 if (k > 0 if bpm == 3 else k >= 4) else 2]
        run = 0
        for v in block[1:]:
            if v == 0:
                run += 1
                continue
            if run > 15:
                lengths.add(int(table[0xF0]))
            lengths.add(int(table[(run & 15) << 4 | abs(v).bit_length()]))
            run = 0
    return lengths


@pytest.mark.parametrize('name', list(C.ROUND_TRIPS))
def test_unscan_inverts_our_own_coder(name):
    video = _video()
    c = C.round_trip(name)
    n_intervals = video.jpeg_layout(c['h'], c['w'], c['subsampling'])[3]
    ranges = C.own_ranges(c['data'], c['offsets'], n_intervals)
    coefficients, status = video.jpeg_unscan(c['data'], ranges, c['h'], c['w'], c['subsampling'])
    assert coefficients.dtype == torch.int16 and status.dtype == torch.int32 and tuple(status.shape) == (c['coefficients'].shape[0], n_intervals)
    assert not status.any() and torch.equal(coefficients, c['coefficients'])
    if name in ('81 MCUs 4:4:4', 'three frames 4:2:0', '19 MCUs 4:2:0'):                # or the case proves less than it claims
        raw = bytes(c['data'].tolist())
        assert b'\xff\x00' in raw and 16 in _ac_code_lengths(c['coefficients'])
    if name == '81 MCUs 4:4:4':
        assert n_intervals == 11 and b'\xff\xd7' in bytes(c['data'].tolist()) and ranges[0, -1, 1] == c['offsets'][-1]
    if name.startswith('19 MCUs'):
        assert n_intervals == 3


@pytest.mark.parametrize('i', range(len(C.FOREIGN_PICTURES) * len(C.FOREIGN_SETTINGS)))
def test_foreign_streams_decode_to_the_first_principles_coefficients(i):
    """... and the coefficients, coded again by the first-principles ENcoder under the stream's own tables and interval, are the stream's scan bytes."""
    label, stream, mode = C.foreign_streams()[i]
    info, coefficients, status = _foreign(i)
    want, want_status, header = C.foreign_reference(i)
    assert not any(want_status) and not status.any(), label
    assert torch.equal(coefficients[0], torch.from_numpy(want)), label
    bpm = coefficients.shape[2]
    blocks = coefficients[0].to(torch.int64).numpy()
    if info.components == 1:
        assert not blocks[:, 1:].any()
        blocks, bpm = blocks[:, :1], 1
    scan, _ = reference_scan(blocks.reshape(-1, 64), bpm, info.restart or blocks.shape[0], info.huffman)
    assert scan == stream[info.scan[0]:info.scan[1]] == split_jpeg(stream)[1], label


def test_foreign_streams_cover_what_they_claim():
    intervals = [_foreign(i)[0].intervals.shape[0] for i in range(len(C.foreign_streams()))]
    infos = [_foreign(i)[0] for i in range(len(C.foreign_streams()))]
    assert max(intervals) > 8 and min(intervals) == 1
    assert {i.subsampling for i in infos} == set(SUBSAMPLINGS) and {i.components for i in infos} == {1, 3}
    assert len({i.huffman for i in infos}) > 10                                     # optimised tables differ from file to file
    assert {i.restart for i in infos} >= {0, 1, 2}


@pytest.mark.parametrize('name', list(PICTURES))
def test_decode_jpeg_shows_what_jpeg_reconstruct_promised(name):
    video = _video()
    x = torch.from_numpy(PICTURES[name])[None]
    for quality in (50, 90):
        for subsampling in SUBSAMPLINGS:
            shown = video.decode_jpeg(video.encode_jpeg(x, quality, subsampling))
            assert shown.dtype == torch.uint8 and torch.equal(shown, video.jpeg_reconstruct(x, quality, subsampling)), (name, quality, subsampling)


def test_a_batch_of_mixed_streams_and_the_files(tmp_path):
    """One call over frames that differ in subsampling, tables and restart interval; load_jpeg; decode_avi and check_avi of a save_avi clip."""
    video = _video()
    picture = PICTURES['gradient']
    x = torch.from_numpy(picture)[None]
    streams = [video.encode_jpeg(x, 90, '4:2:0')[0], C.pillow_jpeg(picture, 'RGB', quality=50, subsampling=0, optimize=True),
               video.encode_jpeg(x, 50, '4:2:0')[0], C.pillow_jpeg(picture, 'L', quality=90, restart_marker_blocks=1),
               C.pillow_jpeg(picture, 'RGB', quality=90, subsampling=2, restart_marker_rows=1, optimize=True)]
    shown, status = video.decode_jpeg(streams, errors='status')
    assert not status.any() and tuple(shown.shape) == (5, 37, 53, 3)
    for i, s in enumerate(streams):
        assert torch.equal(shown[i], video.decode_jpeg([s])[0]), i
    assert torch.equal(shown[0], video.jpeg_reconstruct(x, 90)[0]) and torch.equal(shown[3][..., 0], shown[3][..., 2])
    with pytest.raises(ValueError, match='one size'):
        video.decode_jpeg([streams[0], video.encode_jpeg(torch.from_numpy(PICTURES['noise'])[None])[0]])
    path = tmp_path / 'p.jpg'
    path.write_bytes(streams[1])
    assert torch.equal(video.load_jpeg(path), shown[1])
    clip = torch.from_numpy(np.stack([picture, picture[::-1].copy(), picture[:, ::-1].copy()]))
    video.save_avi(tmp_path / 'c.avi', clip, fps=24, quality=75, subsampling='4:4:4')
    frames, fps = video.decode_avi(tmp_path / 'c.avi')
    assert fps == 24 and torch.equal(frames, video.jpeg_reconstruct(clip, 75, '4:4:4'))
    metrics = video.check_avi(tmp_path / 'c.avi', clip, 75, '4:4:4')
    from pix2pix3d_amd import quality
    assert metrics['exact'] is True and metrics['psnr'] == quality.compare(video.jpeg_reconstruct(clip, 75, '4:4:4'), clip)['psnr']
    assert video.check_avi(tmp_path / 'c.avi', clip, 90, '4:4:4')['exact'] is False


def test_the_pixels_against_libjpeg():
    video = _video()
    worst, lowest = 0, np.inf
    for i, (label, stream, mode) in enumerate(C.foreign_streams()):
        info, coefficients, _ = _foreign(i)
        ours = video.jpeg_decode(coefficients, info.tables, info.h, info.w, info.subsampling)[0].numpy()
        if mode == 'L':
            from PIL import Image
            theirs = np.asarray(Image.open(io.BytesIO(stream)))
            assert np.array_equal(ours[..., 0], ours[..., 1]) and np.array_equal(ours[..., 0], ours[..., 2])
            ours = ours[..., 0]
        else:
            theirs = decode(stream)
        worst = max(worst, int(np.abs(ours.astype(np.int64) - theirs).max()))
        lowest = min(lowest, psnr(ours, theirs))
    print(f'jpeg_decode against libjpeg on {i + 1} streams: at most {worst} grey levels apart, PSNR >= {lowest:.1f} dB')
    record_error('video.jpeg_read.pil_levels', worst)
    record_error('video.jpeg_read.pil_psnr', float(lowest))
    assert worst <= PIL_LEVELS and lowest > 50


def test_jpeg_parse_reads_what_the_segments_say():
    video = _video()
    ours = [video.encode_jpeg(torch.from_numpy(PICTURES['noise'])[None], q, s)[0] for q in (50, 90) for s in SUBSAMPLINGS]
    for stream in ours + [s for _, s, _ in C.foreign_streams()]:
        info, header = video.jpeg_parse(stream), C.header_of(stream)
        assert (info.h, info.w, info.subsampling, info.components, info.restart) == tuple(header[k] for k in ('h', 'w', 'subsampling', 'components', 'restart'))
        assert tuple(tuple(t.tolist()) for t in info.tables) == header['quant'] and all(t.dtype == torch.uint8 for t in info.tables)
        assert info.huffman == header['huffman']
        assert stream[info.scan[0]:info.scan[1]] == header['scan'] and stream[info.scan[1]:info.scan[1] + 2] == b'\xff\xd9'
        n_mcu = video.jpeg_layout(info.h, info.w, info.subsampling)[1]
        assert info.intervals.dtype == np.int64 and info.intervals.shape == (-(-n_mcu // info.restart) if info.restart else 1, 2)
        assert info.intervals[0, 0] == info.scan[0] and info.intervals[-1, 1] == info.scan[1] and np.array_equal(info.intervals[1:, 0], info.intervals[:-1, 1] + 2)
        pieces = [stream[a:b] for a, b in info.intervals.tolist()]
        assert all(b'\xff' not in p.replace(b'\xff\x00', b'') for p in pieces)       # 0xFF 0x00 is data; no marker inside an interval
    for stream in ours:
        assert video.jpeg_parse(stream).restart == video.JPEG_RESTART and video.jpeg_parse(stream).huffman == tuple(zip(video.jpeg_huffman().bits, video.jpeg_huffman().values))


def _with_restarts():
    return C.pillow_jpeg(PICTURES['gradient'], 'RGB', quality=90, subsampling=0, restart_marker_blocks=4)


def _swapped_restarts():
    stream = bytearray(_with_restarts())
    marks = [i for i in range(len(stream) - 1) if stream[i] == 0xFF and 0xD0 <= stream[i + 1] <= 0xD7]
    stream[marks[0] + 1], stream[marks[1] + 1] = stream[marks[1] + 1], stream[marks[0] + 1]
    return bytes(stream)


def _another_interval():
    stream = _with_restarts()
    at = stream.index(b'\xff\xdd\x00\x04\x00\x04')
    return stream[:at + 4] + b'\x00\x05' + stream[at + 6:]


def _over_subscribed():
    video = _video()
    stream = video.encode_jpeg(torch.from_numpy(PICTURES['flat'])[None])[0]
    at = stream.index(b'\xff\xc4\x00\x1f\x00' + bytes(video.jpeg_huffman().bits[0]))
    return stream[:at + 5] + bytes([2, 0, 4, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]) + stream[at + 21:]      # twelve symbols still, two of them 1-bit codes


REFUSALS = {
    'progressive': (lambda: C.pillow_jpeg(PICTURES['gradient'], 'RGB', progressive=True), 'progressive'),
    '4:2:2': (lambda: C.pillow_jpeg(PICTURES['gradient'], 'RGB', subsampling=1), 'sampling factors 2x1 1x1 1x1'),
    'CMYK': (lambda: C.pillow_jpeg(PICTURES['gradient'], 'CMYK'), '4 components'),
    'cut inside its header': (lambda: C.pillow_jpeg(PICTURES['gradient'], 'RGB')[:150], 'ends inside its header'),
    'no EOI': (lambda: C.pillow_jpeg(PICTURES['gradient'], 'RGB')[:-2], 'no EOI'),
    'swapped RST numbers': (_swapped_restarts, 'cyclic order'),
    'another interval count': (_another_interval, '9 restart intervals, but 35 MCUs at an interval of 5 make 7'),
    'an over-subscribed DHT': (_over_subscribed, 'over-subscribe'),
    'not a JPEG': (lambda: b'\x89PNG\r\n\x1a\n' + bytes(40), 'SOI'),
}


@pytest.mark.parametrize('name', list(REFUSALS))
def test_jpeg_parse_refuses_naming_the_cause(name):
    video = _video()
    make, cause = REFUSALS[name]
    stream = make()
    with pytest.raises(ValueError, match=cause):
        video.jpeg_parse(stream)
    with pytest.raises(ValueError, match=cause):
        video.decode_jpeg([stream])


def test_decode_tables_refuse_what_is_no_code():
    video = _video()
    with pytest.raises(ValueError, match='over-subscribe'):
        video.jpeg_decode_tables((3,) + (0,) * 15, (0, 1, 2))
    with pytest.raises(ValueError, match='more than 256'):
        video.jpeg_decode_tables((0,) * 8 + (257,) + (0,) * 7, tuple(range(256)) + (0,))
    with pytest.raises(ValueError, match='16 counts'):
        video.jpeg_decode_tables((1,) * 16, (0, 1))
    words = video.jpeg_decode_tables(*C.header_of(C.foreign_streams()[1][1])['huffman'][2]).numpy().view(np.uint32)
    assert words.shape == (video.JPEG_TABLE_WORDS,) and words[:256].max() >> 16 <= 8


@pytest.mark.parametrize('i', range(20))
def test_damaged_scans_end_in_the_predicted_status(i):
    """The flags are the first-principles decoder's, the intervals that were not touched decode exactly, and what a damaged interval had decoded stays."""
    video = _video()
    label, stream, original = C.damaged_streams()[i]
    want, want_status, _ = C.reference_decode(stream)
    assert any(want_status), label                                                   # every damaged input carries a predicted flag
    frames, status = video.decode_jpeg([stream], errors='status')
    assert status.tolist() == [want_status], (label, status.tolist(), want_status)
    coefficients, unscan_status = video.jpeg_unscan(*C.unscan_arguments(stream))
    assert unscan_status.tolist() == [want_status] and torch.equal(coefficients[0], torch.from_numpy(want)), label
    clean, clean_status = video.jpeg_unscan(*C.unscan_arguments(original))
    assert not clean_status.any()
    info = video.jpeg_parse(stream)
    bpm, restart = coefficients.shape[2], info.restart
    untouched = 0
    for j, (a, b) in enumerate(info.intervals.tolist()):
        a0, b0 = video.jpeg_parse(original).intervals[j].tolist()
        if want_status[j] == 0 and stream[a:b] == original[a0:b0]:
            assert torch.equal(coefficients[0, j * restart:(j + 1) * restart], clean[0, j * restart:(j + 1) * restart]), (label, j)
            untouched += 1
    assert untouched >= len(want_status) - 1 and tuple(frames.shape) == (1, info.h, info.w, 3)
    with pytest.raises(ValueError, match='does not decode'):
        video.decode_jpeg([stream])
    with pytest.raises(ValueError, match='|'.join(video.jpeg_status_names(max(want_status)))):
        video.decode_jpeg([stream], errors='raise')


def test_damage_raises_every_flag_that_bits_can_raise():
    flags = 0
    for _, stream, _ in C.damaged_streams():
        for s in C.reference_decode(stream)[1]:
            flags |= s
    assert flags == C.NO_CODE | C.RUN | C.EXHAUSTED | C.LEFTOVER


def test_a_hostile_table():
    """SIZE needs symbols that no baseline coder emits, so the table is crafted: a DC size of 12, an AC size of 11, an end-of-band run — and ranges that
    lie outside the data, which are clamped."""
    video = _video()
    dc = ((2,) + (0,) * 15, (12, 0))                                               # '0': size 12, '1': size 0
    ac = ((0, 3) + (0,) * 14, (0x0B, 0x50, 0x00))                                   # '00': size 11, '01': EOB5, '10': EOB
    tables = torch.stack([video.jpeg_decode_tables(*t) for t in (dc, dc, ac, ac)])[None]

    def status_of(byte, ranges=((0, 1),)):
        data = torch.tensor([byte], dtype=torch.uint8)
        return video.jpeg_unscan(data, torch.tensor([list(ranges)], dtype=torch.int64), 8, 8, '4:4:4', tables, None, 0, 1)[1].tolist()
    assert status_of(0b00000000) == [[C.SIZE]]                                     # DC size 12
    assert status_of(0b10000000) == [[C.SIZE]]                                     # DC 0, then AC size 11
    assert status_of(0b10100000) == [[C.SIZE]]                                     # DC 0, then EOB5
    assert status_of(0b11011111) == [[0]]                                          # DC 0, EOB, padding
    assert status_of(0b11100000) == [[C.NO_CODE | C.EXHAUSTED]]                    # DC 0, then '11': no code, and fewer than 16 bits were left
    assert status_of(0b11011111, ((-5, 99),)) == [[0]] and status_of(0b11011111, ((7, 3),)) == [[C.EXHAUSTED]]
    coefficients, status = video.jpeg_unscan(torch.tensor([0b11011111] * 4, dtype=torch.uint8), torch.tensor([[[0, 4]]]), 8, 8, '4:4:4', tables, None, 0, 1)
    assert status.tolist() == [[C.LEFTOVER]] and not coefficients.any()


def test_the_routine_under_the_sanitizers(tmp_path):
    """tools/jpeg_unscan_check.cpp — the routine of csrc/video/jpeg_entropy.h, the text a lane of the device kernel runs — built for the host with
    -fsanitize=address,undefined and run as a program of its own on every input of the tests above, damaged ones included: it ends clean (no report, exit
    status 0) with the coefficients and the status of the CPU formulation."""
    video = _video()
    exe, sanitized = C.build_checker(str(tmp_path))
    if not sanitized:
        print('no host compiler links the sanitizer runtimes here: tools/jpeg_unscan_check.cpp ran as a plain build')
    cases = C.all_cases()
    assert len(cases) == len(C.ROUND_TRIPS) + 40 + 20
    results = C.run_checker(exe, cases, str(tmp_path))
    for (label, arguments), (coefficients, status) in zip(cases, results):
        want, want_status = video.jpeg_unscan(*arguments)
        assert torch.equal(status, want_status) and torch.equal(coefficients, want), label
