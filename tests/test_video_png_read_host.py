"""Reading PNG and APNG back (pix2pix3d_amd.video: png_parse, png_inflate, png_unfilter, decode_png and their companions) on the host: the Python
formulation of inflate against ``zlib.decompress`` and against a first-principles decoder (png_read_cases.reference_part: one bit at a time), byte for
byte and status for status — on our own writer's streams with and without the segment index, on Pillow's, on raw zlib streams no PNG writer at hand
makes, and on damaged ones, where the status bits are part of the contract; un-filtering against the filter and against PIL's pixels; the parser's
fields and refusals; and the routine the device runs, built for the host under the address and undefined-behaviour sanitizers and run as a program of
its own on every input above.  Integer equality throughout.  No GPU."""
import io
import zlib

import numpy as np
import pytest
import torch

import png_cases
import png_read_cases as C

FIRST_PRINCIPLES_BYTES = 100_000      # the bit-at-a-time decoder takes the cases up to this size whole, and of a larger one the parts up to it


def _video():
    from pix2pix3d_amd import video
    return video


def test_the_status_bits_are_the_headers():
    video = _video()
    assert video.PNG_STATUS == dict(BLOCK_TYPE=C.BLOCK_TYPE, STORED=C.STORED, CODE_LENGTHS=C.CODE_LENGTHS, NO_CODE=C.NO_CODE, DISTANCE=C.DISTANCE,
                                    OVERFLOW=C.OVERFLOW, EXHAUSTED=C.EXHAUSTED, LEFTOVER=C.LEFTOVER, BOUNDARY=C.BOUNDARY, SHORT=C.SHORT, FILTER=C.FILTER,
                                    ADLER=C.ADLER)
    assert video.png_status_names(C.STORED | C.SHORT) == ['STORED', 'SHORT']
    assert C.CL_ORDER == video.png._CL_ORDER


def test_inflate_equals_zlib_and_the_first_principles_decoder():
    video = _video()
    seen_parts = 0
    for label, data, parts, out_bytes, want in C.clean_cases():
        out, status = video.png_inflate(data, parts, out_bytes)
        assert out.dtype == torch.uint8 and status.dtype == torch.int32 and tuple(status.shape) == (parts.shape[0],), label
        assert not status.any() and bytes(out.tolist()) == want, (label, status.tolist())
        small = parts if out_bytes <= FIRST_PRINCIPLES_BYTES else parts[(parts[:, 3] - parts[:, 2] <= FIRST_PRINCIPLES_BYTES) & (parts[:, 2] < FIRST_PRINCIPLES_BYTES)]
        reference, reference_status = C.reference_inflate(data, small, out_bytes)
        assert not any(reference_status), label
        for _, _, a, b, _ in small.tolist():
            assert reference[a:b] == want[a:b], label
        seen_parts += small.shape[0]
    assert seen_parts > len(C.clean_cases())


def test_the_clean_cases_cover_what_they_claim():
    """Stored, fixed and dynamic blocks, 15-bit codes, the repeat symbols, matches of 258, far distances, a small window, many parts."""
    cases = {label: (data, parts, n) for label, data, parts, n, _ in C.clean_cases()}
    first_byte = {label: int(c[0][0]) for label, c in cases.items()}
    assert first_byte['zlib fixed block'] & 7 == 3 and first_byte['zlib two stored blocks'] & 7 == 0 and first_byte['Pillow RGB default'] & 7 == 5
    assert cases['zlib two stored blocks'][2] == 70000 and cases['own fibonacci index=True frame 0'][1].shape[0] == 71
    assert cases['own three segments index=True frame 0'][1].shape[0] == 3 and cases['zlib full flush, two parts'][1].shape[0] == 2
    assert C.raw_zlib_streams()['window of 512'][0] >> 4 == 1                       # CINFO: a window of 2^(1 + 8)
    files = C.pillow_files()
    assert sum(1 for k, _ in C.chunks_of(files['noise, 5 IDAT']) if k == b'IDAT') == 5
    # the far-match stream really looks 32 340 bytes back: cut off from its first rows it cannot be decoded
    video = _video()
    data, parts, n = cases['zlib far match']
    assert n == 96 * 385
    lengths = _code_lengths_seen(data)
    assert lengths['distance'] >= 32340 and lengths['blocks'] == 2
    seen = [_code_lengths_seen(cases['Pillow RGB ' + k][0]) for k in ('default', 'optimize', 'level 1')]
    assert set().union(*[s['repeats'] for s in seen]) == {16, 17, 18} and all(s['longest code'] >= 11 and s['blocks'] == 1 for s in seen)
    assert max(s['distance'] for s in seen) > 4096
    assert _code_lengths_seen(cases['own fibonacci index=True frame 0'][0], blocks=1)['longest code'] == 15
    assert _code_lengths_seen(cases['Pillow flat'][0])['length'] == 258
    assert video.png_parse(files['P 256']).palette.shape == (256, 3)


def _code_lengths_seen(data, blocks=None):
    """What a stream (or its first ``blocks`` blocks) uses, by a walk of its own over the first-principles tables: the repeat symbols of its headers, its longest code, its longest match
    and its farthest distance, its blocks."""
    raw = bytes(data.tolist())
    seen = {'repeats': set(), 'longest code': 0, 'length': 0, 'distance': 0, 'blocks': 0}
    at = 0

    def bits(n):
        nonlocal at
        v = sum(((raw[(at + i) >> 3] >> ((at + i) & 7)) & 1) << i for i in range(n))
        at += n
        return v

    def symbol(table):
        code = ''
        while code not in table:
            code += str(bits(1))
        return table[code]
    while True:
        last, kind = bits(1), bits(2)
        seen['blocks'] += 1
        if kind == 0:
            at += -at & 7
            at += 32 + 8 * (raw[at >> 3] | raw[(at >> 3) + 1] << 8)
        else:
            if kind == 1:
                lit, dist = C.code_strings([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), C.code_strings([5] * 32)
            else:
                n_lit, n_dist, n_cl = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for s in C.CL_ORDER[:n_cl]:
                    cl[s] = bits(3)
                cl, lengths = C.code_strings(cl), []
                while len(lengths) < n_lit + n_dist:
                    v = symbol(cl)
                    if v < 16:
                        lengths.append(v)
                    else:
                        seen['repeats'].add(v)
                        lengths += [lengths[-1]] * (3 + bits(2)) if v == 16 else [0] * (3 + bits(3) if v == 17 else 11 + bits(7))
                lit, dist = C.code_strings(lengths[:n_lit]), C.code_strings(lengths[n_lit:])
            used = set()
            while True:
                start = at
                v = symbol(lit)
                used.add(at - start)
                if v == 256:
                    break
                if v > 256:
                    seen['length'] = max(seen['length'], png_cases.LENGTH_BASE[v - 257] + bits(png_cases.LENGTH_EXTRA[v - 257]))
                    d = symbol(dist)
                    seen['distance'] = max(seen['distance'], C.DIST_BASE[d] + bits(C.DIST_EXTRA[d]))
            seen['longest code'] = max(seen['longest code'], max(used))
        if last or seen['blocks'] == blocks:
            return seen


@pytest.mark.parametrize('case', range(9))
def test_damaged_streams_end_in_the_predicted_status(case):
    video = _video()
    label, data, parts, out_bytes, want = C.damaged_cases()[case]
    out, status = video.png_inflate(data, parts, out_bytes)
    reference, reference_status = C.reference_inflate(data, parts, out_bytes)
    assert status.tolist() == want == reference_status, (label, status.tolist(), reference_status)
    assert bytes(out.tolist()) == reference, label                                    # what the part had written stays, the rest is zero


def test_there_are_nine_damaged_streams():
    assert len(C.damaged_cases()) == 9


def test_ranges_are_clamped_and_empty_inputs_are_served():
    video = _video()
    label, data, parts, out_bytes, want = C.clean_cases()[0]
    wide = torch.tensor([[-5, 1 << 40, -7, 1 << 40, 1]])
    out, status = video.png_inflate(data, wide, out_bytes)
    assert status.tolist() == [0] and bytes(out.tolist()) == want
    out, status = video.png_inflate(data, torch.tensor([[9, 3, 0, out_bytes, 1]]), out_bytes)         # an end before its begin: no byte
    assert status.tolist() == [C.EXHAUSTED] and not out.any()
    out, status = video.png_inflate(data, torch.zeros([0, 5], dtype=torch.int64), 7)
    assert tuple(out.shape) == (7,) and not out.any() and tuple(status.shape) == (0,)
    with pytest.raises(ValueError, match='parts must be'):
        video.png_inflate(data, torch.zeros([1, 4], dtype=torch.int64), 7)
    with pytest.raises(ValueError, match='data must be'):
        video.png_inflate(data.to(torch.int32), wide, 7)


@pytest.mark.parametrize('bpp', (1, 2, 3, 4))
def test_unfilter_inverts_filter(bpp):
    video = _video()
    rng = np.random.default_rng(60 + bpp)
    x = torch.from_numpy(rng.integers(0, 256, size=[2, 9, 11, bpp] if bpp > 1 else [2, 9, 11], dtype=np.uint8))
    smooth = (x.to(torch.int64) // 16 + torch.arange(11).reshape([1, 1, 11] + [1] * (bpp > 1))).to(torch.uint8)      # rows the adaptive rule treats differently
    for frames in (x, smooth):
        for kind in (0, 1, 2, 3, 4, 'adaptive'):
            filtered = video.png_filter(frames, kind)
            shown, status = video.png_unfilter(filtered, bpp)
            assert not status.any() and shown.dtype == torch.uint8 and torch.equal(shown, frames), (bpp, kind)
            assert np.array_equal(C.reference_unfilter(filtered[1].numpy(), bpp), frames[1].reshape(9, -1).numpy())


@pytest.mark.parametrize('bpp', (1, 3, 6, 8))
def test_unfilter_equals_the_byte_loop(bpp):
    video = _video()
    for kind in (0, 1, 2, 3, 4, 'mix'):
        rows = C.filtered_rows(2, 7, 5, bpp, kind, seed=70 + bpp)
        shown, status = video.png_unfilter(rows, bpp)
        assert not status.any()
        for k in range(2):
            assert np.array_equal(shown[k].reshape(7, -1).numpy(), C.reference_unfilter(rows[k].numpy(), bpp)), (bpp, kind)
    rows = C.filtered_rows(3, 7, 5, bpp, 'mix', seed=80)
    rows[1, 2, 0] = 7
    shown, status = video.png_unfilter(rows, bpp)
    assert status.tolist() == [0, C.FILTER, 0] and np.array_equal(shown[1].reshape(7, -1).numpy(), C.reference_unfilter(rows[1].numpy(), bpp))
    canvas = torch.full([3, 9, 8, bpp] if bpp > 1 else [3, 9, 8], 99, dtype=torch.uint8)
    window = canvas[:, 1:8, 2:7]
    video.png_unfilter(rows, bpp, out=window)
    assert torch.equal(window, shown) and (canvas[:, 0] == 99).all() and (canvas[:, :, :2] == 99).all() and (canvas[:, :, 7:] == 99).all()
    with pytest.raises(ValueError, match='bpp must be'):
        video.png_unfilter(rows, 9)


@pytest.mark.parametrize('label', ['RGB default', 'RGB optimize', 'RGB level 1', 'RGB level 0', 'flat', 'noise, 5 IDAT', 'L', 'LA', 'RGBA', 'P 256', 'I;16'])
def test_pillows_files_decode_to_pils_pixels(label):
    video = _video()
    stream = C.pillow_files()[label]
    frames, status = video.decode_png([stream], errors='status')
    assert not status.any() and tuple(status.shape) == (1, 1)
    assert np.array_equal(frames[0].numpy(), C.pillow_pixels(stream)), label
    info = video.png_parse(stream)
    assert info.delays is None and info.n_plays is None and info.index == [None] and info.streams == [C.zlib_of(stream)]
    if label == 'P 256':
        from PIL import Image
        rgb = np.asarray(Image.open(io.BytesIO(stream)).convert('RGB'))
        assert np.array_equal(video.png_rgb(frames, info)[0].numpy(), rgb)
    if label == 'L':
        assert torch.equal(video.png_rgb(frames, info)[..., 1], frames)


def test_our_own_files_round_trip_with_and_without_the_index():
    video = _video()
    by_label = {}
    for label, mode, frames, palette, index, streams in C.own_files():
        if label.startswith('fibonacci'):
            continue                                                                  # (its inflate is covered above, its decode on the device)
        shown, status = video.decode_png(streams, errors='status')
        assert not status.any() and torch.equal(shown, frames), label
        assert tuple(status.shape) == (frames.shape[0], 3 if label == 'three segments index=True' else 1)
        ignored = video.decode_png(streams, index=False)
        assert torch.equal(ignored, frames)
        by_label[label] = streams
        info = video.png_parse(streams[0])
        assert (info.h, info.w, info.mode) == (frames.shape[1], frames.shape[2], mode) and (info.index[0] is not None) == index
        if mode == 'P':
            assert torch.equal(info.palette, palette) and np.array_equal(video.png_rgb(shown, info)[0].numpy(), png_cases.decode_palette(streams[0]))
        assert video.check_png(streams, frames) and not video.check_png(streams, frames.flip(1))
    for mode in png_cases.MODES:
        plain, indexed = by_label[f'{mode} index=False'], by_label[f'{mode} index=True']
        for a, b in zip(plain, indexed):                                              # the index is one chunk more and nothing else
            assert [c for c in C.chunks_of(b) if c[0] != b'seGM'] == C.chunks_of(a) and len(C.chunks_of(b)) == len(C.chunks_of(a)) + 1
            assert np.array_equal(png_cases.decode(b, mode), png_cases.decode(a, mode))  # Pillow opens an indexed file and shows the picture


def test_the_default_bytes_are_the_parents():
    """``index=False`` changes nothing: the file is the header, ONE IDAT with ``png_deflate``'s stream, IEND — what encode_png wrote before it had the
    argument — and SHA-256 of the six modes' bytes is the value recorded on the parent commit."""
    import hashlib
    video = _video()
    digest = hashlib.sha256()
    for mode in png_cases.MODES:
        frames, palette = png_cases.mode_frames(mode)
        streams = video.encode_png(frames, mode, palette)
        assert streams == video.encode_png(frames, mode, palette, index=False)
        filtered = video.png_filter(frames, 0 if mode == 'P' else 'adaptive')
        data, offsets = video.png_deflate(filtered, video.png_segment_rows(frames.shape[2], png_cases.BPP[mode]))
        for k, stream in enumerate(streams):
            want = video.png_header(frames.shape[1], frames.shape[2], mode, palette) + C.chunk(b'IDAT', bytes(data[offsets[k]:offsets[k + 1]].tolist())) + C.chunk(b'IEND', b'')
            assert stream == want, mode
            digest.update(stream)
    assert digest.hexdigest() == PARENT_DIGEST


PARENT_DIGEST = '730faf2275ec8787c53bc2156d68bb73654c9d81ca47ec51d590d0ea46779336'


def test_the_apng_comes_back_with_its_rate(tmp_path):
    video = _video()
    frames, _ = png_cases.mode_frames('RGB', f=3)
    for index in (False, True):
        video.save_apng(tmp_path / 'a.png', frames, fps=24, loops=2, index=index)
        shown, fps = video.decode_apng(tmp_path / 'a.png')
        assert fps == 24 and type(fps) is int and torch.equal(shown, frames)
        info = video.png_parse((tmp_path / 'a.png').read_bytes())
        assert info.n_plays == 2 and len(info.streams) == 3 and all(d * 24 == 1 for d in info.delays) and all((ix is not None) == index for ix in info.index)
        assert video.check_png(tmp_path / 'a.png', frames)
        theirs, _, _ = png_cases.decode_apng(tmp_path / 'a.png')                       # Pillow plays the indexed file too
        assert all(np.array_equal(a, b.numpy()) for a, b in zip(theirs, frames))
    video.save_apng(tmp_path / 'b.png', frames, fps='30000/1001')
    assert video.decode_apng(tmp_path / 'b.png')[1] * 1001 == 30000
    video.save_png(tmp_path / 'c.png', frames[0], index=True)
    frame, info = video.load_png(tmp_path / 'c.png')
    assert torch.equal(frame, frames[0]) and info.mode == 'RGB' and video.decode_apng(tmp_path / 'c.png')[1] is None


def test_load_mask_and_load_canvas_read_what_the_sessions_save(tmp_path):
    from PIL import Image
    from pix2pix3d_amd import edit, sketch
    mask = np.random.default_rng(81).integers(0, 19, size=[48, 40], dtype=np.uint8)
    Image.fromarray(mask).save(tmp_path / 'mask.png')                               # as EditSession.save and SketchSession.save write them
    Image.fromarray(mask * 13).save(tmp_path / 'canvas.png')
    assert np.array_equal(edit.load_mask(tmp_path / 'mask.png').numpy(), mask)
    assert np.array_equal(sketch.load_canvas(tmp_path / 'canvas.png').numpy(), mask * 13)
    Image.fromarray(np.stack([mask] * 3, axis=2)).save(tmp_path / 'rgb.png')
    with pytest.raises(ValueError, match="mode 'RGB'"):
        edit.load_mask(tmp_path / 'rgb.png')
    with pytest.raises(ValueError, match="mode 'RGB'"):
        sketch.load_canvas(tmp_path / 'rgb.png')


def _ihdr(stream, **fields):
    def change(p):
        p = bytearray(p)
        for k, v in fields.items():
            p[{'depth': 8, 'colour_type': 9, 'interlace': 12}[k]] = v
        return bytes(p)
    return C.replace_chunk(stream, b'IHDR', change)


def _idat(stream, change):
    return C.replace_chunk(stream, b'IDAT', change)


def _without(stream, kind):
    return C.file_of([c for c in C.chunks_of(stream) if c[0] != kind])


def _apng(**changes):
    """An APNG of two frames of ours with one field of its second fcTL (or of a sequence number) changed."""
    import tempfile
    video = _video()
    frames, _ = png_cases.mode_frames('L', f=2)
    with tempfile.TemporaryDirectory() as d:
        video.save_apng(d + '/a.png', frames, fps=10)
        chunks = C.chunks_of(open(d + '/a.png', 'rb').read())
    controls = [i for i, c in enumerate(chunks) if c[0] == b'fcTL']
    p = bytearray(chunks[controls[1]][1])
    for k, v in changes.items():
        if k == 'fdat_sequence':
            at = [i for i, c in enumerate(chunks) if c[0] == b'fdAT'][0]
            chunks[at] = (b'fdAT', v.to_bytes(4, 'big') + chunks[at][1][4:])
        else:
            at, size = {'width': (4, 4), 'x': (12, 4), 'dispose': (24, 1), 'blend': (25, 1)}[k]
            p[at:at + size] = v.to_bytes(size, 'big')
    chunks[controls[1]] = (b'fcTL', bytes(p))
    return C.file_of(chunks)


def _quantized():
    from PIL import Image
    return C.pillow_png(Image.fromarray(C.textured()).quantize(16))


def _rgb16():
    return _ihdr(C.pillow_files()['RGB default'], depth=16)


REFUSALS = {
    'Adam7': (lambda: _ihdr(C.pillow_files()['RGB default'], interlace=1), 'Adam7'),
    'a depth of 4': (_quantized, 'bit depth 4'),
    'a depth of 1': (lambda: _ihdr(C.pillow_files()['L'], depth=1), 'bit depth 1'),
    'a depth of 2': (lambda: _ihdr(C.pillow_files()['L'], depth=2), 'bit depth 2'),
    '16-bit colour': (_rgb16, '16-bit samples other than grey'),
    'not deflate': (lambda: _idat(C.pillow_files()['L'], lambda p: bytes([0x77, 0x01]) + p[2:]), 'not deflate'),
    'a window above 32 K': (lambda: _idat(C.pillow_files()['L'], lambda p: bytes([0x88, 0x1C]) + p[2:]), 'window of at most 32 K'),
    'a preset dictionary': (lambda: _idat(C.pillow_files()['L'], lambda p: bytes([0x78, 0x20]) + p[2:]), 'preset dictionary'),
    'FCHECK': (lambda: _idat(C.pillow_files()['L'], lambda p: bytes([0x78, 0x02]) + p[2:]), 'FCHECK'),
    'a stream of 5 bytes': (lambda: _idat(C.pillow_files()['L'], lambda p: p[:5]), 'shorter than 6'),
    'no IDAT': (lambda: _without(C.pillow_files()['L'], b'IDAT'), 'no IDAT'),
    'no PLTE': (lambda: _without(C.pillow_files()['P 256'], b'PLTE'), 'without PLTE'),
    'PLTE after IDAT': (lambda: C.file_of([c for c in C.chunks_of(C.pillow_files()['P 256']) if c[0] != b'PLTE'][:-1] + [(b'PLTE', bytes(768)), (b'IEND', b'')]),
                        'without PLTE|PLTE after IDAT'),
    'IDAT chunks apart': (lambda: C.file_of(C.chunks_of(C.pillow_files()['L'])[:-1] + [(b'tEXt', b'k\0v'), (b'IDAT', b'xx'), (b'IEND', b'')]), 'IDAT chunks apart'),
    'IHDR of 12 bytes': (lambda: C.replace_chunk(C.pillow_files()['L'], b'IHDR', lambda p: p[:12]), 'IHDR has 12 bytes'),
    'an fcTL of a sub-rectangle': (lambda: _apng(width=5), 'not the whole canvas'),
    'an fcTL at an offset': (lambda: _apng(x=1), 'not the whole canvas'),
    'dispose to background': (lambda: _apng(dispose=1), 'dispose 1 / blend 0'),
    'blend over': (lambda: _apng(blend=1), 'dispose 0 / blend 1'),
    'sequence numbers out of order': (lambda: _apng(fdat_sequence=7), 'sequence numbers out of order'),
    'a bad CRC': (lambda: C.pillow_files()['L'][:-20] + bytes([C.pillow_files()['L'][-20] ^ 1]) + C.pillow_files()['L'][-19:], 'CRC'),
    'an index of the wrong length': (lambda: C.replace_chunk([s for l, *_, s in C.own_files() if l == 'three segments index=True'][0][0], b'seGM', lambda p: p[:-4]),
                                     'seGM lists 2 segments'),
    'not a PNG': (lambda: b'\xff\xd8' + bytes(40), 'signature'),
}


@pytest.mark.parametrize('name', list(REFUSALS))
def test_png_parse_refuses_naming_the_cause(name):
    video = _video()
    make, cause = REFUSALS[name]
    stream = make()
    with pytest.raises(ValueError, match=cause):
        video.png_parse(stream)
    with pytest.raises(ValueError, match=cause):
        video.decode_png([stream])


def test_decode_png_refuses_mixed_sizes_and_bad_arguments():
    video = _video()
    files = C.pillow_files()
    with pytest.raises(ValueError, match='one size and mode'):
        video.decode_png([files['RGB default'], files['L']])
    with pytest.raises(ValueError, match='no stream'):
        video.decode_png([])
    with pytest.raises(ValueError, match="errors is 'raise' or 'status'"):
        video.decode_png([files['L']], errors='ignore')


@pytest.mark.parametrize('case', range(4))
def test_damaged_files_end_in_the_predicted_status(case):
    """A lying index shows as a status — never as a wrong picture that passes for a right one — and the message says what to do; a filter byte of 7 and
    a flipped Adler byte set the frame's bits in column 0."""
    video = _video()
    label, stream, bits = C.damaged_files()[case]
    frames, status = video.decode_png([stream], errors='status')
    if bits is not None:
        assert status.tolist() == [[bits]], (label, status.tolist())
        with pytest.raises(ValueError, match=f'frame 0, part 0 does not decode: {video.png_status_names(bits)[0]}'):
            video.decode_png([stream])
        if bits == C.ADLER:
            assert not video.decode_png([stream], errors='status', verify=False)[1].any()
        return
    info = video.png_parse(stream)
    rows, firsts = info.index[0]
    zstream = info.streams[0]
    _, data, parts, out_bytes, _ = C.case_of(label, zstream, firsts, rows * (1 + 3 * info.w))
    wrong = [j for j in range(parts.shape[0]) if status[0, j] & ~C.ADLER]
    small = parts[wrong]
    reference, reference_status = C.reference_inflate(data, small, out_bytes)
    assert wrong and len(wrong) <= 3 and [int(status[0, j]) & ~C.ADLER for j in wrong] == reference_status and all(reference_status), (label, status.tolist())
    assert int(status[0, 0]) & C.ADLER                                                # and the bytes that did come out are not the stream's
    with pytest.raises(ValueError, match='the index .seGM. does not describe the stream; index=False decodes without it'):
        video.decode_png([stream])
    clean = video.decode_png([stream], index=False)
    assert torch.equal(clean, [frames for l, _, frames, *_ in C.own_files() if l == 'three segments index=True'][0])


def test_the_routine_under_the_sanitizers(tmp_path):
    """tools/png_inflate_check.cpp — the routine of csrc/video/png_inflate.h, the text a lane of the device kernel runs — built for the host with
    -fsanitize=address,undefined and run as a program of its own on every inflate input of the tests above, damaged ones included: it ends clean (no
    report, exit status 0) with the output and the status of the definition."""
    video = _video()
    exe, sanitized = C.build_checker(str(tmp_path))
    if not sanitized:
        print('no host compiler links the sanitizer runtimes here: tools/png_inflate_check.cpp ran as a plain build')
    cases = C.clean_cases() + C.damaged_cases()
    results = C.run_checker(exe, cases, str(tmp_path))
    for (label, data, parts, out_bytes, want), (out, status) in zip(cases, results):
        if isinstance(want, bytes):                                                   # (clean: the definition's output is zlib's, shown above)
            assert not status.any() and bytes(out.numpy()) == want, label
        else:
            definition, definition_status = video.png_inflate(data, parts, out_bytes)
            assert status.tolist() == want and torch.equal(status, definition_status) and torch.equal(out, definition), label
