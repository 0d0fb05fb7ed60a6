"""pix2pix3d_amd.video without a GPU: the torch formulations (the definition of every result byte) against a deliberately slow, loop-written restatement of
the rules, the GIF round trip through PIL, the quality of one global palette against PIL's own per-frame quantiser, the opt-in wiring of generate_video and
the argument checks.  Every comparison of results is integer equality."""
import numpy as np
import pytest
import torch

from model_cases import build_generator
from video_cases import gradient_frames, noise_frames, decode_gif, psnr


# ---- the rules, restated with loops -----------------------------------------------------------------------------------------------------
def slow_histogram(frames):
    counts = [0] * 32768
    for r, g, b in frames.reshape(-1, 3).tolist():
        counts[(r >> 3) << 10 | (g >> 3) << 5 | (b >> 3)] += 1
    return counts


def _bounds(cells):
    return [min(c[a] for c in cells) for a in range(3)], [max(c[a] for c in cells) for a in range(3)]


def slow_median_cut(counts, colors):
    """(boxes as [r_lo, r_hi, g_lo, g_hi, b_lo, b_hi] lists, box_of_bin list): the six steps of video.median_cut over lists of occupied cells."""
    occupied = {(b >> 10, (b >> 5) & 31, b & 31): n for b, n in enumerate(counts) if n}
    if not occupied:
        return [[0] * 6], [0] * 32768
    boxes = [sorted(occupied)]
    while len(boxes) < colors:
        pick = None
        for i, cells in enumerate(boxes):
            lo, hi = _bounds(cells)
            population = sum(occupied[c] for c in cells)
            if lo != hi and (pick is None or population > pick[1]):
                pick = (i, population)
        if pick is None:
            break
        cells, n = boxes[pick[0]], pick[1]
        lo, hi = _bounds(cells)
        axis = 1                                                                  # g, then r, then b: a later one must be strictly longer
        for a in (0, 2):
            if hi[a] - lo[a] > hi[axis] - lo[axis]:
                axis = a
        cum, cut = 0, None
        for s in range(lo[axis], hi[axis] + 1):
            cum += sum(occupied[c] for c in cells if c[axis] == s)
            if 2 * cum >= n:
                cut = s
                break
        cut = min(cut, hi[axis] - 1)
        boxes[pick[0]] = [c for c in cells if c[axis] <= cut]
        boxes.append([c for c in cells if c[axis] > cut])
    box_of = [0] * 32768
    table = []
    for i, cells in enumerate(boxes):
        lo, hi = _bounds(cells)
        table.append([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]])
        for r, g, b in cells:
            box_of[r << 10 | g << 5 | b] = i
    return table, box_of


def slow_box_sums(frames, box_of):
    sums = [[0, 0, 0, 0] for _ in range(256)]
    for r, g, b in frames.reshape(-1, 3).tolist():
        row = sums[box_of[(r >> 3) << 10 | (g >> 3) << 5 | (b >> 3)]]
        row[0] += r
        row[1] += g
        row[2] += b
        row[3] += 1
    return sums


def slow_palette(sums):
    return [[(2 * s + n) // (2 * n) if n else 0 for s in (r, g, b)] for r, g, b, n in sums]


def slow_bayer8():
    m = [[0]]
    for _ in range(3):
        s = len(m)
        m = [[4 * m[y % s][x % s] + ((0, 2), (3, 1))[y // s][x // s] for x in range(2 * s)] for y in range(2 * s)]
    return m


def slow_quantize(frame, palette, n_colors, amplitude):
    b8 = slow_bayer8()
    h, w = len(frame), len(frame[0])
    out = [[0] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            off = ((2 * b8[y & 7][x & 7] - 63) * amplitude) >> 7                   # Python's >> floors, as the rule asks
            p = [min(max(v + off, 0), 255) for v in frame[y][x]]
            best = None
            for k in range(n_colors):
                d2 = sum((p[c] - palette[k][c]) ** 2 for c in range(3))
                if best is None or d2 < best[0]:
                    best = (d2, k)
            out[y][x] = best[1]
    return out


def _counts_of(cells):
    counts = torch.zeros(32768, dtype=torch.int32)
    for (r, g, b), n in cells.items():
        counts[r << 10 | g << 5 | b] = n
    return counts


# ---- formulations -------------------------------------------------------------------------------------------------------------------------
def test_bayer_matrix_is_the_recursion():
    from pix2pix3d_amd import video
    b8 = video.bayer8()
    assert b8.tolist() == slow_bayer8() and sorted(b8.reshape(-1).tolist()) == list(range(64))
    m4 = [[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]]
    assert [[4 * m4[y % 4][x % 4] + ((0, 2), (3, 1))[y // 4][x // 4] for x in range(8)] for y in range(8)] == b8.tolist()
    assert video.dither_offsets(0).abs().max() == 0
    assert (video.dither_offsets(64).min(), video.dither_offsets(64).max()) == (-32, 31)      # (2 B - 63) / 2, floored
    assert (video.dither_offsets(16).min(), video.dither_offsets(16).max()) == (-8, 7)


@pytest.mark.parametrize('per_frame', [False, True])
def test_histogram_and_box_sums_equal_the_loops(per_frame):
    from pix2pix3d_amd import video
    frames = torch.cat([noise_frames(1, 9, 11, seed=1), gradient_frames(2, 9, 11, seed=2)])
    groups = [frames[i:i + 1] for i in range(3)] if per_frame else [frames]
    counts = video.histogram(frames, per_frame)
    assert counts.dtype == torch.int32 and counts.reshape(len(groups), -1).tolist() == [slow_histogram(g) for g in groups]
    cuts = [video.median_cut(c, 16) for c in counts.reshape(len(groups), -1)]
    lookup = torch.stack([b for _, b in cuts])
    sums = video.box_sums(frames, lookup if per_frame else lookup[0], per_frame)
    assert sums.dtype == torch.int64 and tuple(sums.shape) == ((3, 256, 4) if per_frame else (256, 4))
    want = [slow_box_sums(g, lookup[i].tolist()) for i, g in enumerate(groups)]
    assert sums.reshape(len(groups), 256, 4).tolist() == want
    assert video.palette_from_sums(sums).reshape(len(groups), 256, 3).tolist() == [slow_palette(s) for s in want]


def test_pitched_and_strided_frame_views_are_read_in_place():
    from pix2pix3d_amd import video
    canvas = noise_frames(5, 20, 30, seed=3)
    view = canvas[::2, 3:12, 5:16]
    assert not view.is_contiguous()
    assert torch.equal(video.histogram(view), video.histogram(view.contiguous()))
    pal = noise_frames(1, 1, 9, seed=4)[0, 0]
    out = torch.full([3, 12, 16], 255, dtype=torch.uint8)
    got = video.quantize(view, pal, dither=16, out=out[:, 2:11, 4:15])
    assert torch.equal(got, video.quantize(view.contiguous(), pal, dither=16)) and got.data_ptr() == out[:, 2:11, 4:15].data_ptr()
    out[:, 2:11, 4:15] = 255
    assert (out == 255).all()                                                        # nothing around the window was written


MEDIAN_CUT_CASES = {
    # name: (occupied cells -> count, colors, expected boxes or None)
    'a single colour': ({(3, 4, 5): 77}, 256, [[3, 3, 4, 4, 5, 5]]),
    'three cells, 256 colours': ({(0, 0, 0): 5, (10, 2, 0): 1, (31, 31, 31): 9}, 256, None),
    # [10 10 10 10] along r: the first cut leaves two boxes of 20; the tie goes to box 0, whose upper half is appended as box 2
    'a tie in population': ({(0, 0, 0): 10, (1, 0, 0): 10, (2, 0, 0): 10, (3, 0, 0): 10}, 3, [[0, 0, 0, 0, 0, 0], [2, 3, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0]]),
    # extents 3, 3, 3: the cut is on g; 2 cum reaches n = 11 only at the last slice, so it is clamped to the slice before
    'a tie in extent and a clamped cut': ({(0, 0, 0): 5, (3, 3, 3): 5, (0, 3, 0): 1}, 2, [[0, 0, 0, 0, 0, 0], [0, 3, 3, 3, 0, 3]]),
    'a tie in extent between r and b': ({(0, 0, 0): 4, (7, 0, 7): 4}, 2, [[0, 0, 0, 0, 0, 0], [7, 7, 0, 0, 7, 7]]),
    'a clamped cut': ({(0, 0, 0): 1, (5, 0, 0): 100}, 2, [[0, 0, 0, 0, 0, 0], [5, 5, 0, 0, 0, 0]]),
    'nothing occupied': ({}, 4, [[0, 0, 0, 0, 0, 0]]),
}


@pytest.mark.parametrize('name', list(MEDIAN_CUT_CASES))
def test_median_cut_on_planted_histograms(name):
    from pix2pix3d_amd import video
    cells, colors, expected = MEDIAN_CUT_CASES[name]
    counts = _counts_of(cells)
    boxes, box_of = video.median_cut(counts, colors)
    want_boxes, want_box_of = slow_median_cut(counts.tolist(), colors)
    assert boxes.dtype == torch.int32 and box_of.dtype == torch.uint8 and tuple(box_of.shape) == (32768,)
    assert boxes.tolist() == want_boxes and box_of.tolist() == want_box_of
    if expected is not None:
        assert boxes.tolist() == expected
    assert boxes.shape[0] == min(colors, max(len(cells), 1))


@pytest.mark.parametrize('colors', [2, 3, 17, 256])
@pytest.mark.parametrize('kind', ['gradient', 'noise'])
def test_median_cut_equals_the_loops(kind, colors):
    from pix2pix3d_amd import video
    frames = gradient_frames(2, 24, 31, seed=6) if kind == 'gradient' else noise_frames(1, 16, 24, seed=7)
    counts = video.histogram(frames)
    boxes, box_of = video.median_cut(counts, colors)
    want_boxes, want_box_of = slow_median_cut(counts.tolist(), colors)
    assert boxes.tolist() == want_boxes and box_of.tolist() == want_box_of
    assert boxes.shape[0] == min(colors, int((counts > 0).sum()))


QUANTIZE_PALETTE = [[8, 10, 10], [12, 10, 10], [12, 10, 10], [0, 0, 0], [255, 255, 255], [250, 3, 128], [3, 250, 128]]


@pytest.mark.parametrize('dither', [0, 16, 64])
def test_quantize_equals_the_loops(dither):
    """Row 0 and row 1 are equidistant from (10, 10, 10), rows 1 and 2 are the same colour: the lowest index wins both.  Pixels within 32 of 0 and of 255
    meet the clamp under every offset of amplitude 64, and the negative offsets their floor."""
    from pix2pix3d_amd import video
    frames = noise_frames(2, 9, 11, seed=8)
    frames[0, :4] = torch.from_numpy(np.random.default_rng(9).integers(0, 33, size=[4, 11, 3], dtype=np.uint8))
    frames[0, 4:8] = torch.from_numpy(np.random.default_rng(10).integers(223, 256, size=[4, 11, 3], dtype=np.uint8))
    frames[1, :, :4] = torch.tensor([10, 10, 10], dtype=torch.uint8)
    frames[1, :, 4:8] = torch.tensor([12, 10, 10], dtype=torch.uint8)
    palette = torch.tensor(QUANTIZE_PALETTE, dtype=torch.uint8)
    got = video.quantize(frames, palette, dither=dither)
    assert got.dtype == torch.uint8 and got.tolist() == [slow_quantize(f.tolist(), QUANTIZE_PALETTE, 7, dither) for f in frames]
    if dither == 0:
        assert (got[1, :, :4] == 0).all() and (got[1, :, 4:8] == 1).all()
    few = video.quantize(frames, palette, n_colors=3, dither=dither)
    assert few.tolist() == [slow_quantize(f.tolist(), QUANTIZE_PALETTE, 3, dither) for f in frames] and int(few.max()) <= 1
    assert torch.equal(video.quantize(frames, palette, n_colors=torch.tensor([3], dtype=torch.int32), dither=dither), few)
    per_frame = torch.stack([palette, palette.flip(0)])
    got = video.quantize(frames, per_frame, n_colors=torch.tensor([7, 4], dtype=torch.int32), dither=dither, per_frame=True)
    assert got[0].tolist() == slow_quantize(frames[0].tolist(), QUANTIZE_PALETTE, 7, dither)
    assert got[1].tolist() == slow_quantize(frames[1].tolist(), QUANTIZE_PALETTE[::-1], 4, dither)


# ---- partition and means -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['global', 'frame'])
def test_boxes_partition_the_pixels_and_palette_rows_are_their_means(mode):
    from pix2pix3d_amd import video
    frames = gradient_frames(3, 40, 56, seed=11)
    indices, palette, n_colors = video.palettize(frames, colors=64, palette=mode)
    groups = [frames[i:i + 1] for i in range(3)] if mode == 'frame' else [frames]
    assert tuple(palette.shape) == ((3, 256, 3) if mode == 'frame' else (256, 3)) and n_colors.dtype == torch.int32 and n_colors.tolist() == [64] * len(groups)
    for g, group in enumerate(groups):
        counts = video.histogram(group)
        boxes, box_of = video.median_cut(counts, 64)
        sums = video.box_sums(group, box_of)
        assert int(sums[:, 3].sum()) == group.shape[0] * 40 * 56 and (sums[64:] == 0).all()
        cell = torch.arange(32768)
        rgb = torch.stack([cell >> 10, (cell >> 5) & 31, cell & 31], dim=1)
        mine = boxes[box_of.long()].long()
        inside = (rgb[:, 0] >= mine[:, 0]) & (rgb[:, 0] <= mine[:, 1]) & (rgb[:, 1] >= mine[:, 2]) & (rgb[:, 1] <= mine[:, 3]) & (rgb[:, 2] >= mine[:, 4]) & (rgb[:, 2] <= mine[:, 5])
        assert inside[counts > 0].all() and (box_of[counts == 0] == 0).all()
        pixels = group.reshape(-1, 3).long()
        owner = box_of[((pixels[:, 0] >> 3) << 10) | ((pixels[:, 1] >> 3) << 5) | (pixels[:, 2] >> 3)]
        rows = (palette[g] if mode == 'frame' else palette).long()
        for k in range(64):
            own = pixels[owner == k]
            assert len(own) > 0 and rows[k].tolist() == [(2 * int(own[:, c].sum()) + len(own)) // (2 * len(own)) for c in range(3)]
        assert (rows[64:] == 0).all()
        assert torch.equal(indices[g:g + 1] if mode == 'frame' else indices, video.quantize(group, rows[:64].to(torch.uint8)))


# ---- round trip ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['global', 'frame'])
def test_gifs_decode_to_the_palette_rows_of_the_indices(tmp_path, mode):
    from pix2pix3d_amd import video
    frames = gradient_frames(4, 33, 47, seed=12)
    indices, palette, n_colors = video.save_gif(str(tmp_path / 'a.gif'), frames, fps=25, colors=200, dither=16, palette=mode)
    assert n_colors.tolist() == [200] * (4 if mode == 'frame' else 1)
    want = np.stack([(palette[i] if mode == 'frame' else palette).numpy()[indices[i].numpy()] for i in range(4)])
    got = decode_gif(tmp_path / 'a.gif')
    assert got.shape == (4, 33, 47, 3) and np.array_equal(got, want)
    assert psnr(want, frames.numpy()) > 25
    from PIL import Image
    with Image.open(tmp_path / 'a.gif') as im:
        assert im.n_frames == 4 and im.size == (47, 33) and im.info['duration'] == 40 and im.info['loop'] == 0
    short = palette[..., :200, :]                                                # a palette shorter than 256 rows, with a duplicated row
    short = torch.cat([short, short[..., :1, :]], dim=-2)
    video.save_gif_indexed(str(tmp_path / 'b.gif'), indices.numpy(), short, fps=60)
    assert np.array_equal(decode_gif(tmp_path / 'b.gif'), want)


# ---- quality against the current route -----------------------------------------------------------------------------------------------------
def test_one_global_palette_is_no_worse_than_pils_adaptive_palette_per_frame():
    """On smooth gradients with a few grey levels of noise, 4 x 128^2: the global-palette, no-dither PSNR is not below that of PIL's own
    convert('P', palette=ADAPTIVE) per frame (measured with PIL 12.2: 33.70 dB against 32.06 dB)."""
    from PIL import Image
    from pix2pix3d_amd import video
    frames = gradient_frames(4, 128, 128, seed=13)
    indices, palette, _ = video.palettize(frames, colors=256, dither=0, palette='global')
    ours = psnr(palette.numpy()[indices.numpy()], frames.numpy())
    pil = psnr(np.stack([np.asarray(Image.fromarray(f).convert('P', palette=Image.ADAPTIVE).convert('RGB')) for f in frames.numpy()]), frames.numpy())
    print(f'global palette {ours:.2f} dB, PIL adaptive per frame {pil:.2f} dB')
    assert ours >= pil


# ---- wiring ----------------------------------------------------------------------------------------------------------------------------------
def _small(name):
    return build_generator(name, 'cpu', cbase=2048, cmax=32, depth=(6, 6), sr_num_fp16_res=0)


def test_generate_video_writes_a_lossless_label_gif_on_request_and_nothing_else_changes(tmp_path):
    from pix2pix3d_amd import mesh, views
    G = _small('seg2cat')
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(8))
    kw = dict(n_frames=2, views_per_step=2, neural_rendering_resolution=16)
    torch.manual_seed(3)
    before = views.generate_video(G, ws, 'seg2cat', str(tmp_path / 'p.gif'), str(tmp_path / 'pl.gif'), **kw)
    torch.manual_seed(3)
    out = views.generate_video(G, ws, 'seg2cat', str(tmp_path / 'v.gif'), str(tmp_path / 'vl.gif'), gif='device', **kw)
    assert sorted(out) == sorted(before) == ['image', 'label', 'label_index'] and all(torch.equal(out[k], before[k]) for k in out)
    res = G.img_resolution
    label = decode_gif(tmp_path / 'vl.gif')
    assert len(label) <= 2 and all(any(np.array_equal(want, got) for got in label) for want in out['label'].numpy())
    if len(label) == 2:                                                            # (PIL merges frames that are identical)
        assert np.array_equal(label, out['label'].numpy())
    image = decode_gif(tmp_path / 'v.gif')
    assert image.shape[1:] == (res, res, 3) and psnr(image[0], out['image'][0].numpy()) > 20
    assert torch.equal(mesh.default_palette(256)[:7], mesh.default_palette(7))
    with pytest.raises(ValueError):
        views.generate_video(G, ws, 'seg2cat', gif='gpu', **kw)


def test_edge_generators_grey_label_frames_go_through_a_grey_ramp(tmp_path):
    from pix2pix3d_amd import views
    G = _small('edge2car')
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(8))
    out = views.generate_video(G, ws, 'edge2car', None, str(tmp_path / 'l.gif'), n_frames=2, views_per_step=2, neural_rendering_resolution=16, gif='device')
    label = decode_gif(tmp_path / 'l.gif')
    assert out['label'].ndim == 3 and np.array_equal(label[0], np.repeat(out['label'][0].numpy()[..., None], 3, axis=2))


# ---- argument errors ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_raised_before_any_work():
    from pix2pix3d_amd import video
    frames = noise_frames(2, 8, 8)
    pal = torch.zeros([4, 3], dtype=torch.uint8)
    for bad in (frames.float(), frames[..., :2], frames[0], frames.permute(0, 2, 1, 3), frames[:, :, ::2], frames.numpy()):
        for fn in (video.histogram, lambda f: video.quantize(f, pal), lambda f: video.box_sums(f, torch.zeros(32768, dtype=torch.uint8)), video.palettize):
            with pytest.raises(ValueError):
                fn(bad)
    huge = torch.zeros([1, 1, 1, 3], dtype=torch.uint8).expand(2, 32768, 32768, 3)      # 2^31 pixels, one byte of memory
    for fn in (video.histogram, lambda f: video.quantize(f, pal), video.palettize):
        with pytest.raises(ValueError, match='2\\^31'):
            fn(huge)
    for colors in (1, 257, 2.5, True):
        with pytest.raises(ValueError):
            video.median_cut(torch.zeros(32768, dtype=torch.int32), colors)
        with pytest.raises(ValueError):
            video.palettize(frames, colors=colors)
    for amplitude in (-1, 65, 0.5):
        with pytest.raises(ValueError):
            video.quantize(frames, pal, dither=amplitude)
        with pytest.raises(ValueError):
            video.palettize(frames, dither=amplitude)
    for bad_palette in (pal.float(), pal[:, :2], torch.zeros([257, 3], dtype=torch.uint8), torch.zeros([0, 3], dtype=torch.uint8), pal[None]):
        with pytest.raises(ValueError):
            video.quantize(frames, bad_palette)
    with pytest.raises(ValueError):
        video.quantize(frames, pal, n_colors=5)
    with pytest.raises(ValueError):
        video.quantize(frames, pal, out=torch.empty([2, 8, 8], dtype=torch.uint8)[:, :, ::2])
    with pytest.raises(ValueError):
        video.quantize(frames, pal, out=torch.empty([1, 8, 8], dtype=torch.uint8).expand(2, 8, 8))
    with pytest.raises(ValueError):
        video.median_cut(torch.zeros(32767, dtype=torch.int32))
    with pytest.raises(ValueError):
        video.box_sums(frames, torch.zeros(32768, dtype=torch.int32))
    with pytest.raises(ValueError):
        video.palettize(frames, palette='local')
    with pytest.raises(ValueError):
        video.save_gif_indexed('unused.gif', torch.full([1, 4, 4], 9, dtype=torch.uint8), pal)


def test_an_empty_clip_gives_empty_results():
    from pix2pix3d_amd import video
    frames = torch.empty([0, 8, 8, 3], dtype=torch.uint8)
    assert video.histogram(frames).tolist() == [0] * 32768 and tuple(video.histogram(frames, True).shape) == (0, 32768)
    assert tuple(video.quantize(frames, torch.zeros([4, 3], dtype=torch.uint8)).shape) == (0, 8, 8)
    indices, palette, n_colors = video.palettize(frames)
    assert tuple(indices.shape) == (0, 8, 8) and n_colors.tolist() == [1] and (palette == 0).all()
