"""pix2pix3d_amd.video's baseline JPEG and Motion-JPEG AVI on the host: the tables against their formulas and against the files PIL writes, the integer DCT
against fp64, the vectorised entropy coder against a bit-by-bit one on crafted blocks, byte stuffing, every stream decoded by PIL and its PSNR held
against PIL's own encoder with the same tables, the AVI container's structure, and the default path of the video writers unchanged."""
import re
import struct

import numpy as np
import pytest
import torch

from jpeg_cases import (PICTURES, SUBSAMPLINGS, canonical_codes, decode, frames_of, pil_jpeg, psnr, random_coefficients, reference_scan, split_jpeg,
                        tables_of)
from model_cases import build_generator
from pix2pix3d_amd import build
from video_cases import gradient_frames, noise_frames


def _video():
    from pix2pix3d_amd import video
    return video


def _tables():
    h = _video().jpeg_huffman()
    return list(zip(h.bits, h.values))


# ---- tables ----------------------------------------------------------------------------------------------------------------------------------
def test_the_dct_table_equals_its_formula_and_the_header_literals():
    video = _video()
    t = video.jpeg_dct_table()
    u, x = np.mgrid[0:8, 0:8].astype(np.float64)
    want = np.round(8192 * np.where(u == 0, np.sqrt(1 / 8), 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64)
    assert np.array_equal(t.numpy(), want)
    assert t[0].tolist() == [2896] * 8 and t[1, :4].tolist() == [4017, 3406, 2276, 799]
    with open(build.side_paths('video').header) as fh:
        rows = re.findall(r'#define P3D_VIDEO_JPEG_DCT_ROW(\d) (.*)', fh.read())
    assert [int(i) for i, _ in rows] == list(range(8))
    assert [[int(v) for v in row.split(',')] for _, row in rows] == want.tolist()
    z = video.jpeg_zigzag().tolist()
    assert sorted(z) == list(range(64)) and z[:10] == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and z[-3:] == [55, 62, 63]


def test_int32_holds_the_dct_by_the_table_itself():
    t = np.abs(_video().jpeg_dct_table().numpy())
    r = (t.sum(axis=1).max() * 128 + 128) >> 8
    assert r <= 11584
    assert t.sum(axis=1).max() * r + 16384 <= 268378112 + 16384 < 2 ** 31


def test_the_huffman_tables_are_annex_k_and_prefix_free():
    video = _video()
    h = video.jpeg_huffman()
    assert [len(v) for v in h.values] == [12, 12, 162, 162] and [sum(b) for b in h.bits] == [12, 12, 162, 162]
    _, dht = tables_of(pil_jpeg(PICTURES['noise'], 75, '4:2:0'))                  # PIL without `optimize` writes Annex K
    assert [dht[key] for key in (0x00, 0x01, 0x10, 0x11)] == list(zip(h.bits, h.values))
    lookup = h.lookup.numpy().view(np.uint32)
    for t, (bits, values) in enumerate(zip(h.bits, h.values)):
        codes = canonical_codes(bits, values)
        strings = sorted(format(code, f'0{length}b') for code, length in codes.values())
        assert not any(b.startswith(a) for a, b in zip(strings, strings[1:]))      # sorted: a prefix sits right before a string it begins
        assert all(int(lookup[t, s]) == length << 16 | code for s, (code, length) in codes.items())
        assert int((lookup[t] != 0).sum()) == len(values)


@pytest.mark.parametrize('quality', [1, 25, 50, 75, 90, 100])
def test_the_quantisation_tables_equal_the_ones_pil_writes(quality):
    luma, chroma = _video().jpeg_tables(quality)
    dqt, _ = tables_of(pil_jpeg(PICTURES['noise'], quality, '4:2:0'))
    assert luma.dtype == torch.uint8 and tuple(luma.tolist()) == dqt[0] and tuple(chroma.tolist()) == dqt[1]


def test_quality_and_subsampling_are_checked():
    video = _video()
    for bad in (0, 101, 2.5, True):
        with pytest.raises(ValueError):
            video.jpeg_tables(bad)
    with pytest.raises(ValueError):
        video.encode_jpeg(frames_of('flat'), subsampling='4:2:2')
    with pytest.raises(ValueError):
        video.jpeg_scan(torch.zeros([1, 2, 3, 64], dtype=torch.int16), 8, 8, '4:4:4')


# ---- the integer DCT ---------------------------------------------------------------------------------------------------------------------------
def test_the_integer_dct_stays_within_2_of_8_times_the_fp64_dct():
    video = _video()
    rng = np.random.default_rng(41)
    checker = (np.indices([8, 8]).sum(axis=0) % 2) * 255 - 128
    blocks = np.concatenate([rng.integers(-128, 128, size=[200000, 8, 8]), np.full([1, 8, 8], -128), np.full([1, 8, 8], 127), checker[None], -1 - checker[None],
                             rng.choice([-128, 127], size=[100000, 8, 8])]).astype(np.int64)
    got = video.jpeg_dct(torch.from_numpy(blocks)).numpy()
    u, x = np.mgrid[0:8, 0:8].astype(np.float64)
    # 8 a(v) a(u) is applied after the cosine sums, as 1, sqrt(2) or 2: the DC of the fp64 reference is then an exact integer sum.  (The constant block
    # -128 is the extreme: exactly -8192 against -8190, a difference of exactly 2 that a reference rounding a(0)^2 to 0.12500000000000003 reports as more.)
    cosines = np.cos((2 * x + 1) * u * np.pi / 16)
    zero = (np.arange(8) == 0).astype(np.int64)
    scale = np.array([2.0, np.sqrt(2.0), 1.0])[zero[:, None] + zero[None, :]]
    want = scale * (cosines @ blocks.astype(np.float64) @ cosines.T)
    worst = np.abs(got - want).max()
    print(f'integer DCT against 8 x fp64: max difference {worst:.3f}')
    assert worst <= 2


# ---- the entropy coder ---------------------------------------------------------------------------------------------------------------------------
def _scan_equals_the_reference(coefficients, h, w, subsampling):
    video = _video()
    data, offsets = video.jpeg_scan(coefficients, h, w, subsampling)
    assert data.dtype == torch.uint8 and offsets.dtype == torch.int64 and offsets.shape[0] == coefficients.shape[0] + 1 and offsets[-1] == data.shape[0]
    bpm = coefficients.shape[2]
    bits = []
    for i, frame in enumerate(coefficients):
        want, interval_bits = reference_scan(frame.reshape(-1, 64).tolist(), bpm, video.JPEG_RESTART, _tables())
        assert bytes(data[offsets[i]:offsets[i + 1]].tolist()) == want, f'frame {i}'
        bits.append(interval_bits)
    return bytes(data.tolist()), bits


def _blocks(rows):
    return torch.tensor(rows, dtype=torch.int16).reshape(1, 1, len(rows), 64)


def test_all_zero_blocks_are_a_dc_code_and_eob():
    data, _ = _scan_equals_the_reference(_blocks([[0] * 64] * 3), 8, 8, '4:4:4')
    assert data == bytes([0b00101000, 0b00000011])                                 # luma 00 1010, chroma 00 00 twice, two 1-bits of padding


def test_only_coefficient_63_takes_three_zrl_and_no_eob():
    video = _video()
    block = [0] * 63 + [1]
    data, bits = _scan_equals_the_reference(_blocks([block] * 3), 8, 8, '4:4:4')
    codes = [canonical_codes(*t) for t in _tables()]
    luma = codes[0][0][1] + 3 * codes[2][0xF0][1] + codes[2][0xE1][1] + 1            # DC 0, three ZRL, (14, 1), one extra bit
    chroma = codes[1][0][1] + 3 * codes[3][0xF0][1] + codes[3][0xE1][1] + 1
    assert bits == [[luma + 2 * chroma]]
    assert video.JPEG_BLOCK_BITS == 9 + 11 + 63 * 26


def test_the_largest_categories_and_negative_values():
    rows = [[-1024, 1023, -1023, 512, -512, 511, -1] + [0] * 57, [1023, -1023] + [0] * 61 + [-1023], [-1024] + [7, -7] * 31 + [0]]
    rows = rows + [[1016] + [0] * 63, [-1024] + [0] * 63, [1023] + [0] * 63]      # DC differences of category 11, both signs
    _scan_equals_the_reference(torch.tensor(rows, dtype=torch.int16).reshape(1, 2, 3, 64), 8, 16, '4:4:4')
    _scan_equals_the_reference(torch.tensor(rows, dtype=torch.int16).reshape(1, 1, 6, 64), 16, 16, '4:2:0')


def test_black_and_white_blocks_at_quality_100_reach_category_11_and_10():
    video = _video()
    frames = torch.zeros([1, 8, 24, 3], dtype=torch.uint8)
    frames[:, :, 8:16] = 255
    frames[:, :, 20:] = 255                                                        # a block half black, half white
    c = video.jpeg_coefficients(frames, video.jpeg_tables(100), '4:4:4')
    dc = c[0, :, 0, 0].tolist()
    assert dc[0] == -1024 and dc[1] == 1016 and abs(dc[1] - dc[0]).bit_length() == 11
    assert int(c[0, 2, 0, 1:].abs().max()).bit_length() == 10
    _scan_equals_the_reference(c, 8, 24, '4:4:4')


def test_an_interval_whose_bits_end_on_a_byte():
    data, bits = _scan_equals_the_reference(_blocks([[1] + [0] * 63, [0] * 64, [0] * 64]), 8, 8, '4:4:4')
    assert bits == [[16]] and len(data) == 2


@pytest.mark.parametrize('subsampling, h, w', [('4:4:4', 8, 600), ('4:2:0', 16, 1200), ('4:4:4', 24, 200)])
def test_more_than_eight_intervals_wrap_rst_and_the_last_is_shorter(subsampling, h, w):
    video = _video()
    _, n_mcu, bpm, n_intervals = video.jpeg_layout(h, w, subsampling)
    assert n_mcu == 75 and n_intervals == 10 and n_mcu % video.JPEG_RESTART == 3
    coefficients = random_coefficients(2, n_mcu, bpm, seed=42)
    data, bits = _scan_equals_the_reference(coefficients, h, w, subsampling)
    _, offsets = video.jpeg_scan(coefficients, h, w, subsampling)
    frame = data[:int(offsets[1])]
    markers = [frame[i + 1] for i in range(len(frame) - 1) if frame[i] == 0xFF and frame[i + 1] != 0]
    assert markers == [0xD0 + i % 8 for i in range(9)]                              # RST0 .. RST7, RST0; none after the last interval


def test_stuffing_leaves_no_bare_ff():
    video = _video()
    frames = frames_of('noise')
    for subsampling in SUBSAMPLINGS:
        stream, = video.encode_jpeg(frames, 100, subsampling)
        scan = split_jpeg(stream)[1]
        ff = [i for i in range(len(scan)) if scan[i] == 0xFF]
        assert len(ff) >= 3, 'the case must hold 0xFF bytes'
        assert sum(1 for i in ff if i + 1 == len(scan) or not (scan[i + 1] == 0 or 0xD0 <= scan[i + 1] <= 0xD7)) == 0
        assert any(scan[i + 1] == 0 for i in ff)
        c = video.jpeg_coefficients(frames, video.jpeg_tables(100), subsampling)
        _scan_equals_the_reference(c, 24, 40, subsampling)


def test_values_out_of_range_are_clamped_not_miscoded():
    c = _blocks([[3000, -3000, 2000] + [0] * 61, [-3000] + [0] * 63, [0] * 64])
    video = _video()
    data, offsets = video.jpeg_scan(c, 8, 8, '4:4:4')
    want, _ = video.jpeg_scan(c.clamp(-1023, 1023).index_put((torch.tensor([0]), torch.tensor([0]), torch.tensor([1]), torch.tensor([0])),
                                                             torch.tensor(-1024, dtype=torch.int16)), 8, 8, '4:4:4')
    assert torch.equal(data, want)


# ---- whole streams -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
@pytest.mark.parametrize('name', list(PICTURES))
def test_every_stream_decodes_and_holds_pils_psnr(name, subsampling):
    """The PSNR of the decoded stream against the source is at least that of PIL's own encoding with the same tables and subsampling, minus 0.25 dB."""
    video = _video()
    picture = PICTURES[name]
    for quality in (25, 75, 100):
        stream, = video.encode_jpeg(frames_of(name), quality, subsampling)
        markers = [m for m, _ in split_jpeg(stream)[0]]
        assert markers == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
        reference = pil_jpeg(picture, quality, subsampling)
        assert tables_of(stream) == tables_of(reference)
        got = decode(stream)
        assert got.shape == picture.shape
        ours, pils = psnr(got, picture), psnr(decode(reference), picture)
        print(f'{name:14s} {subsampling} quality {quality:3d}: {ours:6.2f} dB, PIL {pils:6.2f} dB, {len(stream)} bytes, PIL {len(reference)}')
        assert ours >= pils - 0.25


def test_the_header_states_the_picture():
    video = _video()
    stream, = video.encode_jpeg(frames_of('gradient'), 90, '4:2:0')
    segments = dict((m, p) for m, p in split_jpeg(stream)[0] if m not in (0xDB, 0xC4))
    assert segments[0xE0][:5] == b'JFIF\0'
    assert segments[0xC0] == bytes([8, 0, 37, 0, 53, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert segments[0xDD] == struct.pack('>H', video.JPEG_RESTART)
    assert segments[0xDA] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert split_jpeg(video.encode_jpeg(frames_of('gradient'), 90, '4:4:4')[0])[0][3][1][7] == 0x11


def test_frames_in_place_numpy_input_and_no_frames():
    video = _video()
    frames = torch.cat([gradient_frames(3, 37, 53, seed=43), noise_frames(1, 37, 53, seed=44)])
    want = video.encode_jpeg(frames, 75)
    canvas = noise_frames(5, 40, 60, seed=45)
    canvas[1:, 2:39, 3:56] = frames
    assert video.encode_jpeg(canvas[1:, 2:39, 3:56], 75) == want
    assert video.encode_jpeg(frames.numpy()[::2], 75) == want[::2] == video.encode_jpeg(frames[::2], 75)
    assert video.encode_jpeg(torch.empty([0, 16, 16, 3], dtype=torch.uint8)) == []
    c = video.jpeg_coefficients(torch.empty([0, 16, 16, 3], dtype=torch.uint8), video.jpeg_tables(90))
    assert tuple(c.shape) == (0, 0, 6, 64)
    data, offsets = video.jpeg_scan(c, 16, 16)
    assert data.numel() == 0 and offsets.tolist() == [0]


def test_save_jpeg_writes_one_still(tmp_path):
    video = _video()
    stream = video.save_jpeg(tmp_path / 'still.jpg', frames_of('gradient')[0], quality=95, subsampling='4:4:4')
    assert (tmp_path / 'still.jpg').read_bytes() == stream == video.encode_jpeg(frames_of('gradient'), 95, '4:4:4')[0]
    assert psnr(decode(stream), PICTURES['gradient']) > 35


# ---- the container -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fps', [60, 24, 29.97])
def test_the_avi_is_well_formed_and_read_avi_follows_its_index(tmp_path, fps):
    video = _video()
    frames = torch.cat([gradient_frames(3, 37, 53, seed=46), noise_frames(2, 37, 53, seed=47)])
    path = tmp_path / 'clip.avi'
    returned = video.save_avi(path, frames, fps=fps, quality=75, subsampling='4:4:4')
    streams = video.encode_jpeg(frames, 75, '4:4:4')
    assert returned == streams and any(len(s) % 2 for s in streams)                 # at least one chunk needs its padding byte
    data = path.read_bytes()
    assert data[:4] == b'RIFF' and struct.unpack('<I', data[4:8])[0] == len(data) - 8 and data[8:12] == b'AVI '
    assert data[12:16] == b'LIST' and data[20:24] == b'hdrl' and data[24:28] == b'avih' and struct.unpack('<I', data[28:32])[0] == 56
    avih = struct.unpack('<14I', data[32:88])
    assert avih[0] == round(1e6 / fps) and avih[3] & 0x10 and avih[4] == 5 and avih[6] == 1 and avih[8:10] == (53, 37)
    assert data[88:92] == b'LIST' and data[96:100] == b'strl' and data[100:104] == b'strh' and data[108:116] == b'vidsMJPG'
    strf = data.index(b'strf')
    size, w, h, planes, bit_count, compression = struct.unpack('<IiiHH4s', data[strf + 8:strf + 28])
    assert struct.unpack('<I', data[strf + 4:strf + 8])[0] == 40 and (size, w, h, planes, bit_count, compression) == (40, 53, 37, 1, 24, b'MJPG')
    movi = data.index(b'movi')
    idx1 = data.index(b'idx1', movi + sum(len(s) for s in streams))
    assert struct.unpack('<I', data[idx1 + 4:idx1 + 8])[0] == 16 * 5 and idx1 + 8 + 16 * 5 == len(data)
    at = movi + 4
    for i, s in enumerate(streams):
        fourcc, flags, offset, size = struct.unpack('<4sIII', data[idx1 + 8 + 16 * i:idx1 + 24 + 16 * i])
        assert fourcc == b'00dc' and flags & 0x10 and size == len(s) and movi + offset == at and at % 2 == 0
        assert data[at:at + 4] == b'00dc' and struct.unpack('<I', data[at + 4:at + 8])[0] == size and data[at + 8:at + 8 + size] == s
        at += 8 + size + size % 2
    assert at == idx1
    got, got_fps, size = video.read_avi(path)
    assert got == streams and got_fps == pytest.approx(fps, rel=1e-6) and size == (53, 37)
    assert all(psnr(decode(s), f.numpy()) > 25 for s, f in zip(got[:3], frames[:3]))


def test_an_avi_needs_a_frame_and_stays_below_2_gib(tmp_path, monkeypatch):
    video = _video()
    with pytest.raises(ValueError):
        video.save_avi(tmp_path / 'none.avi', torch.empty([0, 8, 8, 3], dtype=torch.uint8))
    monkeypatch.setattr(video.avi, 'MAX_AVI_BYTES', 2000)
    with pytest.raises(ValueError):
        video.save_avi(tmp_path / 'large.avi', noise_frames(2, 24, 40), quality=100)
    assert not (tmp_path / 'none.avi').exists() and not (tmp_path / 'large.avi').exists()
    (tmp_path / 'not.avi').write_bytes(b'RIFF\x04\0\0\0WAVE')
    with pytest.raises(ValueError):
        video.read_avi(tmp_path / 'not.avi')


# ---- the video writers ---------------------------------------------------------------------------------------------------------------------------
def _small(name):
    return build_generator(name, 'cpu', cbase=2048, cmax=32, depth=(6, 6), sr_num_fp16_res=0)


def test_generate_video_keeps_its_gif_bytes_and_writes_avis_on_request(tmp_path):
    from pix2pix3d_amd import views
    video = _video()
    G = _small('seg2cat')
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(8))
    kw = dict(n_frames=2, views_per_step=2, neural_rendering_resolution=16)
    names = {}
    for tag, extra in (('plain', {}), ('gif', {'format': 'gif'}), ('avi', {'format': 'avi'})):
        torch.manual_seed(3)
        ext = extra.get('format', 'gif')
        names[tag] = (tmp_path / f'{tag}_image.{ext}', tmp_path / f'{tag}_label.{ext}')
        out = views.generate_video(G, ws, 'seg2cat', str(names[tag][0]), str(names[tag][1]), **kw, **extra)
    for a, b in zip(names['plain'], names['gif']):
        assert a.read_bytes() == b.read_bytes() and a.read_bytes()[:6] == b'GIF89a'
    for path, frames in zip(names['avi'], (out['image'], out['label'])):
        streams, fps, size = video.read_avi(path)
        assert streams == video.encode_jpeg(frames) and fps == 60 and size == (frames.shape[2], frames.shape[1])
    with pytest.raises(ValueError):
        views.generate_video(G, ws, 'seg2cat', format='mp4', **kw)


def test_generate_video_writes_the_edge_generators_grey_labels_as_an_avi(tmp_path):
    from pix2pix3d_amd import views
    video = _video()
    G = _small('edge2car')
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(8))
    out = views.generate_video(G, ws, 'edge2car', None, str(tmp_path / 'l.avi'), n_frames=2, views_per_step=2, neural_rendering_resolution=16, format='avi')
    streams, _, _ = video.read_avi(tmp_path / 'l.avi')
    assert out['label'].ndim == 3 and streams == video.encode_jpeg(out['label'][..., None].expand(-1, -1, -1, 3).contiguous())


def test_geometry_video_takes_the_format_keyword():
    import inspect
    from pix2pix3d_amd import surface, views
    for fn in (surface.geometry_video, views.generate_video):
        p = inspect.signature(fn).parameters
        assert p['format'].default == 'gif' and list(p).index('format') == list(p).index('gif') + 1
