"""pix2pix3d_amd.video's PNG and APNG writers on the host: every zlib stream inflated by zlib itself (which also checks the combined Adler-32), every file decoded
by PIL to exactly the frame that went in, the adaptive filter against a byte-by-byte formulation, the token counts against the stream definition worded as a
loop, the length-limited code against a heapq Huffman and Kraft's sum, the APNG container, and the default paths of the writers unchanged."""
import inspect
import zlib

import numpy as np
import pytest
import torch

from model_cases import build_generator
from png_cases import (BPP, MODES, chunk_straddlers, crafted_rows, decode, decode_apng, decode_palette, fibonacci_counts, fibonacci_frame, filter_pictures,
                       huffman_lengths, mode_frames, picture_frames, reference_filter, reference_filter_row, reference_stats)
from video_cases import gradient_frames, noise_frames


def _video():
    from pix2pix3d_amd import video
    return video


def _inflates_to(data, offsets, filtered):
    for i in range(filtered.shape[0]):
        stream = bytes(data[offsets[i]:offsets[i + 1]].tolist())
        assert stream[:2] == b'\x78\x01'
        assert zlib.decompress(stream) == filtered[i].numpy().tobytes(), f'frame {i}'


# ---- whole files -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('filter', [None, 0, 1, 2, 3, 4, 'adaptive'])
@pytest.mark.parametrize('mode', MODES)
def test_every_mode_and_filter_inflates_and_decodes_to_the_frame(mode, filter):
    video = _video()
    frames, palette = mode_frames(mode)
    filt = (0 if mode == 'P' else 5) if filter is None else filter
    filtered = video.png_filter(frames, filt)
    assert tuple(filtered.shape) == (2, 13, 1 + 37 * BPP[mode])
    want_types = {filt} if filt not in (5, 'adaptive') else set(range(5))
    assert set(filtered[:, :, 0].reshape(-1).tolist()) <= want_types
    _inflates_to(*video.png_deflate(filtered, video.png_segment_rows(37, BPP[mode])), filtered)
    files = video.encode_png(frames, mode if mode in ('P', 'I;16') else None, palette, filter)
    assert len(files) == 2
    for stream, frame in zip(files, frames):
        chunks = video.png_chunks(stream)
        assert [k for k, _ in chunks] == ([b'IHDR', b'PLTE', b'IDAT', b'IEND'] if mode == 'P' else [b'IHDR', b'IDAT', b'IEND'])
        assert np.array_equal(decode(stream, mode), frame.numpy())
        if mode == 'P':
            assert np.array_equal(decode_palette(stream), palette.numpy()[frame.numpy()])


def test_sixteen_bit_depth_reads_back_as_its_values():
    video = _video()
    depth = torch.linspace(0.5, 3.5, 7 * 9, dtype=torch.float32).reshape(1, 7, 9)
    depth[0, 0, :3] = torch.tensor([-1.0, 99.0, float('nan')])
    pairs = video.depth16(depth, 1.0, 3.0)
    want = np.floor((depth.double().numpy() - 1.0) / 2.0 * 65535 + 0.5)
    want = np.nan_to_num(want, nan=0.0).clip(0, 65535).astype(np.int64)
    assert pairs.dtype == torch.uint8 and tuple(pairs.shape) == (1, 7, 9, 2)
    assert np.array_equal(pairs[..., 0].numpy().astype(np.int64) << 8 | pairs[..., 1].numpy(), want) and want[0, 0, :3].tolist() == [0, 65535, 0]
    from PIL import Image
    import io
    stream, = video.encode_png(pairs, 'I;16')
    with Image.open(io.BytesIO(stream)) as im:
        assert np.array_equal(np.asarray(im).astype(np.int64), want[0])
    with pytest.raises(ValueError):
        video.depth16(depth, 2.0, 2.0)


def test_frames_in_place_numpy_input_no_frames_and_bad_arguments(tmp_path):
    video = _video()
    frames = torch.cat([gradient_frames(3, 37, 53, seed=43), noise_frames(1, 37, 53, seed=44)])
    want = video.encode_png(frames)
    canvas = noise_frames(5, 40, 60, seed=45)
    canvas[1:, 2:39, 3:56] = frames
    assert video.encode_png(canvas[1:, 2:39, 3:56]) == want
    assert video.encode_png(frames.numpy()[::2]) == want[::2] == video.encode_png(frames[::2])
    assert video.encode_png(torch.empty([0, 16, 16, 3], dtype=torch.uint8)) == []
    assert video.save_png(tmp_path / 'one.png', frames[1]) == want[1] == (tmp_path / 'one.png').read_bytes()
    paths = video.save_png_sequence(str(tmp_path / 'f_{:03d}.png'), frames)
    assert paths == [str(tmp_path / f'f_{i:03d}.png') for i in range(4)] and [open(p, 'rb').read() for p in paths] == want
    filtered = video.png_filter(torch.empty([2, 0, 5, 3], dtype=torch.uint8))
    assert tuple(filtered.shape) == (2, 0, 16)
    data, offsets = video.png_deflate(filtered, 4)
    assert data.numel() == 0 and offsets.tolist() == [0, 0, 0] and tuple(video.png_counts(filtered, 4).shape) == (2, 0, video.PNG_STATS)
    for bad in (lambda: video.encode_png(frames, 'P'), lambda: video.encode_png(frames, palette=torch.zeros([4, 3], dtype=torch.uint8)),
                lambda: video.encode_png(frames[..., 0], 'P', torch.zeros([257, 3], dtype=torch.uint8)), lambda: video.encode_png(frames, 'I;16'),
                lambda: video.encode_png(frames.float()), lambda: video.encode_png(frames, filter=6), lambda: video.encode_png(frames, filter='best'),
                lambda: video.encode_png(torch.empty([1, 0, 4, 3], dtype=torch.uint8)), lambda: video.png_deflate(video.png_filter(frames), 0),
                lambda: video.encode_png(frames.permute(0, 2, 1, 3)), lambda: video.png_header(0, 4, 'RGB'), lambda: video.png_header(4, 4, 'CMYK')):
        with pytest.raises(ValueError):
            bad()


def test_png_chunks_refuses_a_damaged_file():
    video = _video()
    stream, = video.encode_png(gradient_frames(1, 9, 11, seed=46))
    assert [k for k, _ in video.png_chunks(stream)] == [b'IHDR', b'IDAT', b'IEND']
    ihdr = video.png_chunks(stream)[0][1]
    assert ihdr == (11).to_bytes(4, 'big') + (9).to_bytes(4, 'big') + bytes([8, 2, 0, 0, 0])
    damaged = bytearray(stream)
    damaged[40] ^= 1
    for bad in (bytes(damaged), stream[:-5], stream + b'\0', b'GIF89a' + stream[6:]):
        with pytest.raises(ValueError):
            video.png_chunks(bad)


# ---- the container -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fps', [60, 50, 24, 29.97])
def test_the_apng_plays_back_every_frame_exactly(tmp_path, fps):
    video = _video()
    frames = torch.cat([gradient_frames(3, 21, 33, seed=47), noise_frames(2, 21, 33, seed=48)])
    path = tmp_path / 'clip.png'
    streams = video.save_apng(path, frames, fps=fps, loops=3)
    got, durations, loop = decode_apng(path)
    assert len(got) == 5 and loop == 3 and all(np.array_equal(g, f.numpy()) for g, f in zip(got, frames))
    assert all(d == pytest.approx(1000 / fps, rel=1e-4) for d in durations)
    chunks = video.png_chunks(path.read_bytes())
    assert [k for k, _ in chunks] == [b'IHDR', b'acTL', b'fcTL', b'IDAT'] + [b'fcTL', b'fdAT'] * 4 + [b'IEND']
    assert chunks[1][1] == (5).to_bytes(4, 'big') + (3).to_bytes(4, 'big')
    numbered = [p for k, p in chunks if k in (b'fcTL', b'fdAT')]
    assert [int.from_bytes(p[:4], 'big') for p in numbered] == list(range(9))      # one running sequence number
    control = chunks[2][1]
    assert control[4:20] == (33).to_bytes(4, 'big') + (21).to_bytes(4, 'big') + bytes(8) and control[24:26] == bytes(2)
    num, den = int.from_bytes(control[20:22], 'big'), int.from_bytes(control[22:24], 'big')
    assert num / den == pytest.approx(1 / fps, rel=1e-6)
    assert [chunks[3][1]] + [p[4:] for k, p in chunks if k == b'fdAT'] == streams
    first, = video.encode_png(frames[:1])
    assert video.png_chunks(first)[1] == chunks[3]                                   # a viewer without APNG sees frame 0


def test_an_apng_of_indices_keeps_them_and_needs_a_frame(tmp_path):
    video = _video()
    indices, palette = mode_frames('P', f=3)
    video.save_apng(tmp_path / 'p.png', indices, fps=30, mode='P', palette=palette)
    got, _, loop = decode_apng(tmp_path / 'p.png')
    assert loop == 0 and all(np.array_equal(g, palette.numpy()[i.numpy()]) for g, i in zip(got, indices))
    assert [k for k, _ in video.png_chunks(tmp_path / 'p.png')][:3] == [b'IHDR', b'PLTE', b'acTL']
    for bad in (lambda: video.save_apng(tmp_path / 'none.png', torch.empty([0, 8, 8, 3], dtype=torch.uint8)),
                lambda: video.save_apng(tmp_path / 'none.png', indices, fps=0), lambda: video.save_apng(tmp_path / 'none.png', indices, fps=1e-6),
                lambda: video.save_apng(tmp_path / 'none.png', indices, loops=-1)):
        with pytest.raises(ValueError):
            bad()
    assert not (tmp_path / 'none.png').exists()


# ---- the filter ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['L', 'LA', 'RGB', 'RGBA'])
def test_the_adaptive_filter_equals_a_byte_by_byte_formulation(mode):
    video = _video()
    frames, _ = mode_frames(mode, f=2, h=9, w=14)
    got = video.png_filter(frames)
    for i in range(2):
        assert np.array_equal(got[i].numpy(), reference_filter(frames[i].numpy(), BPP[mode])), f'frame {i}'       # a frame's first row sees zeros above


def test_a_tie_goes_to_the_lower_type():
    video = _video()
    row = [5 * x for x in range(12) for _ in range(3)]
    above = [0] * 36
    costs = []
    for kind in range(5):                                                          # above a first row, Paeth predicts what Sub predicts
        filtered = video.png_filter(torch.tensor(row, dtype=torch.uint8).reshape(1, 1, 12, 3), kind)[0, 0, 1:].tolist()
        costs.append(sum(r if r < 128 else 256 - r for r in filtered))
    assert costs[1] == costs[4] == min(costs) and costs[0] > costs[1]
    assert reference_filter_row(row, above, 3)[0] == 1
    assert video.png_filter(torch.tensor(row, dtype=torch.uint8).reshape(1, 1, 12, 3))[0, 0, 0] == 1
    assert video.png_filter(torch.zeros([1, 3, 5, 3], dtype=torch.uint8))[0, :, 0].tolist() == [0, 0, 0]      # all five tie


def test_the_adaptive_rule_chooses_each_of_the_five_types():
    video = _video()
    chosen = {}
    for name in filter_pictures():
        frames = picture_frames(name)
        filtered = video.png_filter(frames)
        assert np.array_equal(filtered[0].numpy(), reference_filter(frames[0].numpy(), 3)), name
        chosen[name] = set(filtered[0, :, 0].tolist())
    print(chosen)
    assert set().union(*chosen.values()) == {0, 1, 2, 3, 4}
    assert 2 in chosen['horizontal ramp'] and 4 in chosen['diagonal ramp'] and 0 in chosen['noise'] and 3 in chosen['gradient and noise']


# ---- tokens and counts -----------------------------------------------------------------------------------------------------------------------------
def _stats_equal_the_reference(filtered, segment_rows):
    video = _video()
    stats = video.png_counts(filtered, segment_rows)
    f, h, r = filtered.shape
    assert stats.dtype == torch.int32 and tuple(stats.shape) == (f, -(-h // segment_rows), video.PNG_STATS)
    for i in range(f):
        for s in range(stats.shape[1]):
            segment = filtered[i, s * segment_rows:(s + 1) * segment_rows].reshape(-1).tolist()
            assert stats[i, s].tolist() == reference_stats(segment), (i, s)
    return stats


def test_the_counts_of_every_way_a_run_can_end():
    video = _video()
    rows = crafted_rows()
    stats = _stats_equal_the_reference(video.png_filter(rows, 0), 1)
    # m = 258: one match; 259: and a literal; 260: and two; 261: 258 + 3; 518: 258 + 258 + two literals
    assert stats[:, 0, 285].tolist() == [1, 1, 1, 1, 2] and stats[:, 0, 257].tolist() == [0, 0, 0, 1, 0]
    assert stats[:, 0, 253].tolist() == [1, 2, 3, 1, 3] and stats[:, 0, 287].tolist() == [1, 1, 1, 2, 2]
    _inflates_to(*video.png_deflate(video.png_filter(rows, 0), 1), video.png_filter(rows, 0))


def test_the_counts_of_runs_around_the_walks_steps_and_of_plain_pictures():
    video = _video()
    for frames, filt, rows in ((chunk_straddlers(), 0, 1), (picture_frames('gradient and noise'), 5, 5), (picture_frames('vertical ramp'), 0, 24),
                               (torch.full([1, 20, 300], 9, dtype=torch.uint8), 0, 7), (torch.full([1, 20, 300], 9, dtype=torch.uint8), 2, 3)):
        filtered = video.png_filter(frames, filt)
        _stats_equal_the_reference(filtered, rows)
        _inflates_to(*video.png_deflate(filtered, rows), filtered)


def test_segments_are_coded_on_their_own():
    """Every segment but the last ends in an empty stored block on a byte boundary; one row a segment over 70 rows, and a shorter last segment."""
    video = _video()
    frames = gradient_frames(2, 70, 19, seed=49)
    filtered = video.png_filter(frames)
    for rows, n_seg in ((1, 70), (4, 18), (70, 1), (1000, 1)):
        data, offsets = video.png_deflate(filtered, rows)
        _inflates_to(data, offsets, filtered)
        assert video.png_counts(filtered, rows).shape[1] == n_seg
        assert bytes(data[offsets[0]:offsets[1]].tolist()).count(b'\x00\x00\xff\xff') >= n_seg - 1
    filtered = video.png_filter(gradient_frames(1, 10, 19, seed=50))
    _stats_equal_the_reference(filtered, 4)                                        # 4 + 4 + 2 rows
    _inflates_to(*video.png_deflate(filtered, 4), filtered)


# ---- the code --------------------------------------------------------------------------------------------------------------------------------------
def _kraft(lengths):
    return sum(2 ** (15 - int(v)) for v in lengths if v)


def test_code_lengths_are_complete_limited_and_as_cheap_as_huffman():
    video = _video()
    rng = np.random.default_rng(74)
    histograms = [rng.integers(0, 1000, size=286), rng.integers(0, 3, size=286), (rng.random(286) ** 8 * 1e6).astype(np.int64), np.arange(286), [1, 1],
                  [5, 0, 0, 9], [1] * 286, [0] * 100 + [7, 7, 7], 2 ** np.arange(12), fibonacci_counts(20)]
    for counts in histograms:
        counts = np.asarray(counts, dtype=np.int64)
        lengths = video.png_code_lengths(counts)
        assert lengths.shape == counts.shape and ((lengths > 0) == (counts > 0)).all() and lengths.max() <= 15
        assert _kraft(lengths) == 2 ** 15
        plain = huffman_lengths(counts)
        if max(plain.values()) <= 15:
            assert int((lengths * counts).sum()) == sum(counts[s] * d for s, d in plain.items())
        codes = video.png_canonical_codes(lengths)
        strings = sorted(format(int(c), f'0{int(n)}b') for c, n in zip(codes, lengths) if n)
        assert not any(b.startswith(a) for a, b in zip(strings, strings[1:]))        # prefix-free
    assert video.png_code_lengths([0, 0, 4, 0]).tolist() == [0, 0, 1, 0] and video.png_code_lengths([0, 0, 0]).tolist() == [0, 0, 0]
    assert video.png_code_lengths([3, 1, 1, 1], limit=2).tolist() == [2, 2, 2, 2]
    with pytest.raises(ValueError):
        video.png_code_lengths([1] * 5, limit=2)
    assert video.png_canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]).tolist() == [2, 3, 4, 5, 6, 0, 14, 15]      # RFC 1951's own example


def test_a_fibonacci_histogram_is_limited_to_15_bits_and_still_decodes():
    video = _video()
    counts = np.zeros(286, dtype=np.int64)
    counts[1:31] = fibonacci_counts(30)
    assert max(huffman_lengths(counts).values()) == 29
    lengths = video.png_code_lengths(counts)
    assert lengths.max() == 15 and _kraft(lengths) == 2 ** 15
    assert int((lengths * counts).sum()) > sum(counts[s] * d for s, d in huffman_lengths(counts).items())      # the limit costs something
    assert video.png_code_lengths(counts, limit=29).max() == 29 and \
        int((video.png_code_lengths(counts, limit=29) * counts).sum()) == sum(counts[s] * d for s, d in huffman_lengths(counts).items())
    frames = fibonacci_frame()
    filtered = video.png_filter(frames, 0)
    rows = video.png_segment_rows(frames.shape[2], 1)
    stats = video.png_counts(filtered, rows)
    frame_counts = stats[0, :, :286].sum(dim=0).numpy().astype(np.int64)
    frame_counts[256] = stats.shape[1]
    assert max(huffman_lengths(frame_counts).values()) > 15
    used = video.png_code_lengths(frame_counts)
    assert used[1] == 15 and used.max() == 15
    # the head: the type byte, then the values 1 and 2 in turn, none a run — the bits before the k-th 15-bit code are known, and some straddle a 32-bit word
    _, header_bits = video.png_block_header(used)
    at = [1 + header_bits + int(used[0]) + k * int(used[1] + used[2]) for k in range(64)]
    assert any(a % 32 > 17 for a in at) and any(a % 32 <= 17 for a in at)
    data, offsets = video.png_deflate(filtered, rows)
    _inflates_to(data, offsets, filtered)
    stream, = video.encode_png(frames, filter=0)
    assert np.array_equal(decode(stream, 'L'), frames[0].numpy())


def test_the_block_header_is_what_zlib_reads():
    """A block of the header, one literal and end of block inflates to that literal, for codes from flat to deep."""
    video = _video()
    for counts in ([3] * 286, [0] * 65 + [9] + [0] * 190 + [1] + [0] * 29, list(range(1, 287)), [0] * 256 + [1] + [0] * 28 + [5]):
        counts = np.asarray(counts, dtype=np.int64)
        lengths = video.png_code_lengths(counts)
        codes = video.png_canonical_codes(lengths)
        bits, n = video.png_block_header(lengths)
        assert bits < 1 << n <= 1 << (32 * video.PNG_HEADER_WORDS) and bits & 3 == 2
        symbol = int(np.flatnonzero(lengths[:256])[0]) if lengths[:256].any() else None
        stream, at = 1 | bits << 1, 1 + n
        for s in ([symbol] if symbol is not None else []) + [256]:
            for bit in range(int(lengths[s]) - 1, -1, -1):                          # a code goes in from its most significant bit
                stream |= ((int(codes[s]) >> bit) & 1) << at
                at += 1
        raw = stream.to_bytes((at + 7) // 8, 'little')
        assert zlib.decompressobj(-15).decompress(raw) == (bytes([symbol]) if symbol is not None else b'')


# ---- the writers -------------------------------------------------------------------------------------------------------------------------------------
def _small(name):
    return build_generator(name, 'cpu', cbase=2048, cmax=32, depth=(6, 6), sr_num_fp16_res=0)


def test_generate_video_keeps_its_gifs_and_writes_apngs_on_request(tmp_path):
    from pix2pix3d_amd import mesh, views
    G = _small('seg2cat')
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(8))
    kw = dict(n_frames=2, views_per_step=2, neural_rendering_resolution=16)
    names = {}
    for tag, extra in (('gif', {}), ('apng', {'format': 'apng'})):
        torch.manual_seed(3)
        ext = {'gif': 'gif', 'apng': 'png'}[extra.get('format', 'gif')]
        names[tag] = (tmp_path / f'{tag}_image.{ext}', tmp_path / f'{tag}_label.{ext}')
        out = views.generate_video(G, ws, 'seg2cat', str(names[tag][0]), str(names[tag][1]), **kw, **extra)
        if tag == 'gif':                                                             # the default: the bytes mesh.save_gif writes of the same frames, as before
            for path, key in zip(names[tag], ('image', 'label')):
                mesh.save_gif(str(tmp_path / 'direct.gif'), out[key], fps=60)
                assert path.read_bytes() == (tmp_path / 'direct.gif').read_bytes() and path.read_bytes()[:6] == b'GIF89a'
    image, durations, _ = decode_apng(names['apng'][0])
    assert all(np.array_equal(g, f.numpy()) for g, f in zip(image, out['image'])) and durations == [pytest.approx(1000 / 60)] * 2
    from PIL import Image
    palette = mesh.default_palette(256).numpy()
    with Image.open(names['apng'][1]) as im:
        assert im.mode == 'P' and im.n_frames == 2
        for i in range(2):
            im.seek(i)
            assert np.array_equal(np.asarray(im), out['label_index'][i].numpy())     # the indices themselves, and through the palette the label frames
            assert np.array_equal(np.asarray(im.convert('RGB')), out['label'][i].numpy()) and np.array_equal(palette[np.asarray(im)], out['label'][i].numpy())
    with pytest.raises(ValueError):
        views.generate_video(G, ws, 'seg2cat', format='mp4', **kw)


def test_generate_video_writes_the_edge_generators_grey_labels_as_an_apng(tmp_path):
    from pix2pix3d_amd import views
    video = _video()
    G = _small('edge2car')
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(8))
    out = views.generate_video(G, ws, 'edge2car', None, str(tmp_path / 'l.png'), n_frames=2, views_per_step=2, neural_rendering_resolution=16, format='apng')
    assert out['label'].ndim == 3 and video.png_chunks(tmp_path / 'l.png')[0][1][8:10] == bytes([8, 0])      # 8-bit grey
    got, _, _ = decode_apng(tmp_path / 'l.png')
    assert all(np.array_equal(g, f.numpy()) for g, f in zip(got, out['label']))


def test_generate_sample_writes_its_pngs_where_the_frames_are_on_request(tmp_path):
    from PIL import Image
    from pix2pix3d_amd import views
    G = _small('seg2cat')
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(8))
    camera = views.video_cameras(G, 'seg2cat', 2)[0]
    kw = dict(neural_rendering_resolution=16)
    files = {}
    for tag, extra in (('pil', {}), ('device', {'png': 'device'})):
        torch.manual_seed(3)
        files[tag] = (tmp_path / f'{tag}_c.png', tmp_path / f'{tag}_l.png')
        out = views.generate_sample(G, ws, camera, str(files[tag][0]), str(files[tag][1]), **kw, **extra)
    with Image.open(files['pil'][1]) as x:
        assert x.mode == 'RGB'                                                       # the default stays PIL's file of the RGB label frame
    assert inspect.signature(views.generate_sample).parameters['png'].default == 'pil'
    for (a, b), key in zip(zip(files['pil'], files['device']), ('image', 'label')):
        with Image.open(a) as x, Image.open(b) as y:
            assert np.array_equal(np.asarray(x.convert('RGB')), np.asarray(y.convert('RGB'))) and np.array_equal(np.asarray(y.convert('RGB')), out[key][0].numpy())
    with Image.open(files['device'][1]) as y:
        assert y.mode == 'P' and np.array_equal(np.asarray(y), out['label_index'][0].numpy())
    assert list(inspect.signature(views.generate_sample).parameters)[-2:] == ['png', 'synthesis_kwargs']
    with pytest.raises(ValueError):
        views.generate_sample(G, ws, camera, png='host', **kw)


def test_the_format_keyword_keeps_its_place_and_mp4_keeps_raising():
    from pix2pix3d_amd import surface, views
    for fn in (surface.geometry_video, views.generate_video):
        p = inspect.signature(fn).parameters
        assert p['format'].default == 'gif' and list(p).index('format') == list(p).index('gif') + 1
    G = _small('seg2cat')
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(8))
    with pytest.raises(ValueError):
        surface.geometry_video(G, ws, 'seg2cat', format='mp4')
