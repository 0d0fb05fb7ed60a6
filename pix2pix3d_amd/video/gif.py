"""Colour-quantised video frames on the frames' own device, and GIFs written from them.

``mesh.save_gif`` hands RGB frames to PIL, which picks a palette per frame and maps every pixel to it on one CPU core before the LZW coding: that, not
the rendering, is what a caller of ``views.generate_video`` waits for.  Here the colour work is four integer steps (csrc/video/p3d_video.h states the
rules; libp3d_video.so, a library of its own like the region tools'), each with a torch formulation that CPU tensors take — the definition — and, for the
three that touch every pixel, device kernels whose bytes equal it:

    histogram(frames)                     int32 [32768] (or [F, 32768]): pixels per bin of 5 bits a channel, bin = (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3)
    median_cut(counts, colors)            boxes int32 [K, 6] and the bin -> box lookup uint8 [32768]; always on the host, over the 32^3 cells
    box_sums(frames, box_of_bin)          int64 [256, 4] (or [F, 256, 4]): the sums of r, g, b over the 8-bit colours of every box, and their number
    palette_from_sums(sums)               uint8 [K, 3]: the rounded mean colour of every box
    quantize(frames, palette, ...)        uint8 [F, H, W]: the nearest palette row by squared distance, the lowest on a tie, after an 8 x 8 ordered dither

``palettize`` runs them in order, ``save_gif_indexed`` writes index frames and their palette as a GIF without any further quantisation, and ``save_gif``
is the two together.  Frames are uint8 [F, H, W, 3] with contiguous pixels (``stride(3) == 1``, ``stride(2) == 3``) and any row and frame pitch: a strided
selection ``frames[::4]`` and a window of a larger canvas are read in place.  One palette serves the whole clip (``per_frame=False``) or one frame
(``per_frame=True``).  ``palette_quality`` measures what the knobs cost (``quality.py``; DESIGN.md sections 2.1q and 2.1x)."""
import numpy as np
import torch

from .. import _lib
from .. import quality as Q
from ..clips import HEADER, check, check_frames, clip_args, video_lib

BINS, COLORS, MAX_AMPLITUDE = (HEADER.constants[k] for k in ('P3D_VIDEO_BINS', 'P3D_VIDEO_COLORS', 'P3D_VIDEO_MAX_AMPLITUDE'))


def _bins(frames):
    v = frames.to(torch.int64) >> 3
    return (v[..., 0] << 10) | (v[..., 1] << 5) | v[..., 2]


# ---- histogram -------------------------------------------------------------------------------------------------------------------------
def histogram(frames, per_frame=False):
    """int32 [32768], or [F, 32768] with ``per_frame``: the number of pixels in every bin.  Device tensors: ``p3d_video_histogram`` (the histogram of a
    work-group in LDS, flushed with integer atomics); CPU tensors: ``bincount``."""
    f, h, w = check_frames(frames)
    groups = f if per_frame else 1
    if f * h * w == 0:
        counts = torch.zeros([groups, BINS], dtype=torch.int32, device=frames.device)
    elif not frames.is_cuda:
        bins = _bins(frames).reshape(groups, -1)
        counts = torch.stack([torch.bincount(row, minlength=BINS) for row in bins]).to(torch.int32)
    else:
        counts = torch.empty([groups, BINS], dtype=torch.int32, device=frames.device)
        with _lib.kernel_timer('video_histogram', counts):
            code = video_lib().p3d_video_histogram(*clip_args(frames), int(bool(per_frame)), _lib.ptr(counts), _lib.stream_of(counts))
        check(code, 'video_histogram')
    return counts if per_frame else counts[0]


# ---- median cut ------------------------------------------------------------------------------------------------------------------------
_AXIS_ORDER = (1, 0, 2)                              # ties in extent: g, r, b


def _tight(cells, lo, hi):
    """The box [lo, hi] (inclusive, per axis) shrunk to the occupied cells inside it, and their population.  The box holds at least one."""
    sub = cells[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
    new_lo, new_hi = [], []
    for axis in range(3):
        on = np.flatnonzero(sub.sum(axis=tuple(a for a in range(3) if a != axis)))
        new_lo.append(lo[axis] + int(on[0]))
        new_hi.append(lo[axis] + int(on[-1]))
    return new_lo, new_hi, int(sub.sum())


def median_cut(counts, colors=COLORS):
    """(boxes int32 [K, 6], box_of_bin uint8 [32768]) of one histogram ``counts`` [32768], 2 <= ``colors`` <= 256, on the host (a device histogram is copied:
    128 KB, one synchronisation).  A box is (r_lo, r_hi, g_lo, g_hi, b_lo, b_hi), inclusive, in cells of 8 grey levels.  The rule:

    1. the first box is the tight bounds of the occupied cells (of an empty histogram: the cell 0, and K = 1);
    2. while there are fewer than ``colors`` boxes and some box spans more than one cell on some axis, take, among those boxes, the one with the largest
       population, the lowest index on a tie;
    3. cut it on its longest axis, ties in the order g, r, b;
    4. after the smallest slice s with 2 cum(s) >= n (cum: the population up to and including s, n: the box's), but not after the last one: the upper
       part is never empty;
    5. the lower part keeps the box's index, the upper part is appended;
    6. both shrink to tight bounds.

    K < ``colors`` when fewer cells are occupied.  ``box_of_bin`` maps an occupied cell to its box and every empty cell to 0."""
    if isinstance(colors, bool) or int(colors) != colors or not 2 <= int(colors) <= COLORS:
        raise ValueError(f'median_cut: colors must be an integer 2 .. {COLORS}, got {colors!r}')
    if not torch.is_tensor(counts) or counts.dtype not in (torch.int32, torch.int64) or tuple(counts.shape) != (BINS,):
        raise ValueError(f'median_cut: counts must be an int32 [{BINS}] tensor')
    cells = counts.detach().cpu().numpy().astype(np.int64).reshape(32, 32, 32)
    if (cells < 0).any():
        raise ValueError('median_cut: counts must be >= 0')
    box_of = np.zeros([32, 32, 32], dtype=np.uint8)
    if not cells.any():
        return torch.zeros([1, 6], dtype=torch.int32), torch.from_numpy(box_of.reshape(-1))
    lo, hi, n = _tight(cells, [0, 0, 0], [31, 31, 31])
    boxes = [(lo, hi, n)]
    while len(boxes) < colors:
        pick = None
        for i, (lo, hi, n) in enumerate(boxes):
            if lo != hi and (pick is None or n > boxes[pick][2]):
                pick = i
        if pick is None:
            break
        lo, hi, n = boxes[pick]
        axis = max(_AXIS_ORDER, key=lambda a: hi[a] - lo[a])                      # max keeps the first of equal keys: g, r, b
        sub = cells[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
        cum = np.cumsum(sub.sum(axis=tuple(a for a in range(3) if a != axis)))
        s = min(int(np.argmax(2 * cum >= n)), hi[axis] - lo[axis] - 1)
        lower_hi, upper_lo = list(hi), list(lo)
        lower_hi[axis], upper_lo[axis] = lo[axis] + s, lo[axis] + s + 1
        boxes[pick] = _tight(cells, lo, lower_hi)
        boxes.append(_tight(cells, upper_lo, hi))
    for i, (lo, hi, _) in enumerate(boxes):
        box_of[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = i
    box_of[cells == 0] = 0
    table = torch.tensor([[lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]] for lo, hi, _ in boxes], dtype=torch.int32)
    return table, torch.from_numpy(box_of.reshape(-1))


# ---- box sums and the palette ----------------------------------------------------------------------------------------------------------
def box_sums(frames, box_of_bin, per_frame=False):
    """int64 [256, 4], or [F, 256, 4] with ``per_frame``: per box the sums of r, g and b over the true 8-bit colours of the pixels whose bin maps to it, and
    their number n.  ``box_of_bin`` uint8 [32768] (or [F, 32768]) on the frames' device.  Device tensors: ``p3d_video_box_sums`` (the lookup and the 256
    accumulators in LDS, one flush per work-group); CPU tensors: ``index_add_``."""
    f, h, w = check_frames(frames)
    groups = f if per_frame else 1
    if not torch.is_tensor(box_of_bin) or box_of_bin.dtype != torch.uint8 or tuple(box_of_bin.shape) != ((groups, BINS) if per_frame else (BINS,)):
        raise ValueError(f'box_sums: box_of_bin must be uint8 {[groups, BINS] if per_frame else [BINS]}')
    if box_of_bin.device != frames.device:
        raise ValueError(f'box_sums: box_of_bin is on {box_of_bin.device}, the frames on {frames.device}')
    lookup = box_of_bin.reshape(groups, BINS).contiguous()
    if f * h * w == 0:
        sums = torch.zeros([groups, COLORS, 4], dtype=torch.int64, device=frames.device)
    elif not frames.is_cuda:
        sums = torch.zeros([groups, COLORS, 4], dtype=torch.int64)
        bins, pixels = _bins(frames).reshape(groups, -1), frames.reshape(groups, -1, 3).to(torch.int64)
        for g in range(groups):
            rows = torch.cat([pixels[g], torch.ones_like(pixels[g][:, :1])], dim=1)
            sums[g].index_add_(0, lookup[g][bins[g]].long(), rows)
    else:
        sums = torch.empty([groups, COLORS, 4], dtype=torch.int64, device=frames.device)
        with _lib.kernel_timer('video_box_sums', sums):
            code = video_lib().p3d_video_box_sums(*clip_args(frames), int(bool(per_frame)), _lib.ptr(lookup), _lib.ptr(sums), _lib.stream_of(sums))
        check(code, 'video_box_sums')
    return sums if per_frame else sums[0]


def palette_from_sums(sums):
    """uint8 [..., K, 3] of int64 ``sums`` [..., K, 4]: every channel the rounded mean (2 sum + n) // (2 n); a box without pixels gets black.  Torch ops on the
    sums' device, no synchronisation."""
    if not torch.is_tensor(sums) or sums.dtype != torch.int64 or sums.ndim < 2 or sums.shape[-1] != 4:
        raise ValueError('palette_from_sums: sums must be an int64 [..., K, 4] tensor')
    n = sums[..., 3:]
    return torch.where(n > 0, (2 * sums[..., :3] + n) // (2 * n).clamp(min=1), 0).to(torch.uint8)


# ---- quantize ------------------------------------------------------------------------------------------------------------------------------
def bayer8():
    """int64 [8, 8]: the Bayer matrix of the recursion M <- [[4M, 4M+2], [4M+3, 4M+1]] from [[0]], three steps."""
    m = torch.zeros([1, 1], dtype=torch.int64)
    for _ in range(3):
        m = torch.cat([torch.cat([4 * m, 4 * m + 2], dim=1), torch.cat([4 * m + 3, 4 * m + 1], dim=1)], dim=0)
    return m


def dither_offsets(amplitude):
    """int64 [8, 8]: what the ordered dither adds to every channel of the pixel (x, y), at [y & 7][x & 7]: ((2 B8 - 63) * amplitude) >> 7, a floor."""
    return ((2 * bayer8() - 63) * int(amplitude)) >> 7


def _check_amplitude(dither):
    if isinstance(dither, bool) or int(dither) != dither or not 0 <= int(dither) <= MAX_AMPLITUDE:
        raise ValueError(f'dither (the amplitude) must be an integer 0 .. {MAX_AMPLITUDE}, got {dither!r}')
    return int(dither)


_CHUNK = 1 << 16                                     # pixels per step of the CPU formulation: 64 MB of int32 keys


def _quantize_torch(frames, palette, n_colors, amplitude, out):
    f, h, w = frames.shape[:3]
    off = dither_offsets(amplitude).repeat((h + 7) // 8, (w + 7) // 8)[:h, :w].reshape(-1, 1)
    k = torch.arange(COLORS, dtype=torch.int64)
    for i in range(f):
        g = i if palette.shape[0] > 1 else 0
        rows, n = palette[g].to(torch.int64), int(n_colors[g].clamp(1, COLORS))
        pixels = (frames[i].reshape(-1, 3).to(torch.int64) + off).clamp(0, 255)
        index = torch.empty([h * w], dtype=torch.uint8)
        for p0 in range(0, h * w, _CHUNK):
            d2 = ((pixels[p0:p0 + _CHUNK, None, :] - rows[None, :n, :]) ** 2).sum(dim=2)
            index[p0:p0 + _CHUNK] = ((d2 << 8) | k[:n]).min(dim=1).values & 255                # ordered by (d^2, k): the lowest k on a tie
        out[i].copy_(index.view(h, w))
    return out


def quantize(frames, palette, n_colors=None, dither=0, per_frame=False, out=None):
    """uint8 [F, H, W]: for every pixel the row of ``palette`` nearest to its dithered colour.  ``palette`` uint8 [K, 3], 1 <= K <= 256 (``per_frame``:
    [F, K, 3]) on the frames' device; ``n_colors`` None (all K rows count), an int, or an int32 tensor [1] / [F] on the frames' device — it is read where
    the frames are and clamped to 1 .. K, so a palette made on the device needs no synchronisation.  ``dither``: the amplitude, 0 .. 64, 0 for none.  Per
    pixel (x, y) and channel v' = clamp(v + off, 0, 255), off = ((2 B8[y & 7][x & 7] - 63) * dither) >> 7 (``dither_offsets``); the index is the
    k < n_colors that minimises dr^2 + dg^2 + db^2, the lowest such k.  ``out``: the caller's uint8 [F, H, W] view with contiguous pixels and any pitches
    (bytes around it stay untouched).  Device tensors: ONE ``p3d_video_quantize`` launch; CPU tensors: the torch formulation."""
    f, h, w = check_frames(frames)
    amplitude = _check_amplitude(dither)
    groups = f if per_frame else 1
    if not torch.is_tensor(palette) or palette.dtype != torch.uint8 or palette.ndim != (3 if per_frame else 2) or palette.shape[-1] != 3 \
            or not 1 <= palette.shape[-2] <= COLORS or (per_frame and palette.shape[0] != f):
        raise ValueError(f'quantize: palette must be uint8 {"[F, K, 3]" if per_frame else "[K, 3]"} with 1 <= K <= {COLORS}')
    if palette.device != frames.device:
        raise ValueError(f'quantize: the palette is on {palette.device}, the frames on {frames.device}')
    k = palette.shape[-2]
    if n_colors is None or not torch.is_tensor(n_colors):
        n = k if n_colors is None else int(n_colors)
        if not 1 <= n <= k:
            raise ValueError(f'quantize: n_colors must be 1 .. {k}, got {n_colors!r}')
        n_colors = torch.full([groups], n, dtype=torch.int32, device=frames.device)
    elif n_colors.dtype != torch.int32 or tuple(n_colors.shape) != (groups,) or n_colors.device != frames.device:
        raise ValueError(f'quantize: n_colors must be an int32 [{groups}] tensor on {frames.device}')
    if out is None:
        out = torch.empty([f, h, w], dtype=torch.uint8, device=frames.device)
    elif not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (f, h, w) or out.device != frames.device:
        raise ValueError(f'quantize: out must be uint8 [{f}, {h}, {w}] on {frames.device}')
    elif f * h * w and (out.stride(2) != 1 or out.stride(1) < w or (f > 1 and out.stride(0) < h * out.stride(1))):
        raise ValueError(f'quantize: out needs contiguous pixels and rows and frames that do not overlap, got strides {tuple(out.stride())}')
    if f * h * w == 0:
        return out
    full = torch.zeros([groups, COLORS, 3], dtype=torch.uint8, device=frames.device)       # the kernel's palette: 256 rows a group
    full[:, :k] = palette.reshape(groups, k, 3)
    n_colors = n_colors.clamp(1, k).contiguous()
    if not frames.is_cuda:
        return _quantize_torch(frames, full, n_colors, amplitude, out)
    with _lib.kernel_timer('video_quantize', out):
        code = video_lib().p3d_video_quantize(*clip_args(frames), int(bool(per_frame)), _lib.ptr(full), _lib.ptr(n_colors), amplitude, _lib.ptr(out),
                                              out.stride(0), out.stride(1), _lib.stream_of(out))
    check(code, 'video_quantize')
    return out


# ---- the four steps ------------------------------------------------------------------------------------------------------------------------
def palettize(frames, colors=COLORS, dither=0, palette='global'):
    """``(indices uint8 [F, H, W], palette uint8 [256, 3], n_colors int32 [1])`` for ``palette='global'`` — one palette for the clip, so flat areas do not
    shimmer from frame to frame — or ``(indices, palette [F, 256, 3], n_colors [F])`` for ``'frame'``, all on the frames' device.  The four steps: histogram,
    median cut to at most ``colors`` (2 .. 256) boxes, box means, nearest-row indices under the ordered dither of amplitude ``dither``.  Rows from
    ``n_colors`` on are zeros and never chosen.  The median cut runs on the host: the histogram (128 KB a group) is copied there and the lookup (32 KB a
    group) back — the ONLY synchronisation with the host; everything per pixel stays on the frames' device."""
    f, h, w = check_frames(frames)
    if palette not in ('global', 'frame'):
        raise ValueError(f"palettize: palette must be 'global' or 'frame', got {palette!r}")
    if isinstance(colors, bool) or int(colors) != colors or not 2 <= int(colors) <= COLORS:
        raise ValueError(f'palettize: colors must be an integer 2 .. {COLORS}, got {colors!r}')
    _check_amplitude(dither)
    per_frame = palette == 'frame'
    groups = f if per_frame else 1
    counts = histogram(frames, per_frame).reshape(groups, BINS).cpu()
    cuts = [median_cut(c, colors) for c in counts]
    lookup = torch.stack([box_of for _, box_of in cuts]).to(frames.device) if groups else torch.zeros([0, BINS], dtype=torch.uint8, device=frames.device)
    n_colors = torch.tensor([boxes.shape[0] for boxes, _ in cuts], dtype=torch.int32).to(frames.device)
    sums = box_sums(frames, lookup if per_frame else lookup[0], per_frame)
    pal = palette_from_sums(sums)                                                        # rows past a group's K have n = 0: zeros
    return quantize(frames, pal, n_colors, dither, per_frame), pal, n_colors


def save_gif_indexed(path, indices, palette, fps=60):
    """Index frames uint8 [F, H, W] and their palette uint8 [K, 3] (or one a frame, [F, K, 3]), K <= 256, as a GIF that loops forever: one 'P' image per frame
    with ``putpalette``, no quantisation anywhere; the frame duration is ``mesh.save_gif``'s, max(1, round(1000 / fps)) ms.  Decoded, every frame equals
    ``palette[indices]`` exactly.  As with ``mesh.save_gif``, PIL merges consecutive IDENTICAL frames into one with a longer duration, so a clip that stands
    still decodes to fewer frames of the same total length.  Tensors on any device (they are copied to the host) or numpy arrays."""
    from PIL import Image
    idx = torch.as_tensor(indices).detach().cpu()
    pal = torch.as_tensor(palette).detach().cpu()
    if idx.dtype != torch.uint8 or idx.ndim != 3 or idx.shape[0] < 1:
        raise ValueError('save_gif_indexed: indices must be uint8 [F, H, W] with F >= 1')
    if pal.dtype != torch.uint8 or pal.ndim not in (2, 3) or pal.shape[-1] != 3 or not 1 <= pal.shape[-2] <= COLORS or (pal.ndim == 3 and pal.shape[0] != idx.shape[0]):
        raise ValueError(f'save_gif_indexed: palette must be uint8 [K, 3] or [{idx.shape[0]}, K, 3] with 1 <= K <= {COLORS}')
    if idx.numel() and int(idx.max()) >= pal.shape[-2]:
        raise ValueError(f'save_gif_indexed: an index reaches {int(idx.max())} with {pal.shape[-2]} palette rows')
    idx, pal = idx.contiguous().numpy(), pal.contiguous().numpy()
    images = []
    for i, a in enumerate(idx):
        im = Image.fromarray(a, 'P')
        im.putpalette((pal[i] if pal.ndim == 3 else pal).tobytes())
        images.append(im)
    images[0].save(path, save_all=True, append_images=images[1:], duration=max(1, round(1000 / fps)), loop=0)


def save_gif(path, frames, fps=60, colors=COLORS, dither=16, palette='global'):
    """``palettize`` then ``save_gif_indexed``: RGB frames uint8 [F, H, W, 3], on the device or the host, as a GIF.  Returns what ``palettize`` returned."""
    frames = torch.as_tensor(frames)
    result = palettize(frames, colors, dither, palette)
    save_gif_indexed(path, result[0], result[1], fps=fps)
    return result


def palette_quality(frames, indices, palette):
    """``quality.compare`` of what a GIF shows, ``palette[indices]``, against the frames it was made from — what ``colors``, ``dither`` and ``palette`` of
    ``palettize`` cost.  ``indices`` uint8 [F, H, W], ``palette`` uint8 [K, 3] or [F, K, 3], on the frames' device; one gather there, two launches, ONE host read."""
    f, h, w = check_frames(frames)
    if not torch.is_tensor(indices) or indices.dtype != torch.uint8 or tuple(indices.shape) != (f, h, w) or indices.device != frames.device:
        raise ValueError(f'palette_quality: indices must be uint8 [{f}, {h}, {w}] on {frames.device}')
    if not torch.is_tensor(palette) or palette.dtype != torch.uint8 or palette.ndim not in (2, 3) or palette.shape[-1] != 3 or palette.device != frames.device \
            or (palette.ndim == 3 and palette.shape[0] != f):
        raise ValueError(f'palette_quality: palette must be uint8 [K, 3] or [{f}, K, 3] on {frames.device}')
    idx = indices.long().clamp(max=palette.shape[-2] - 1)                        # (an index past the palette shows its last row: no read out of bounds)
    shown = palette[idx] if palette.ndim == 2 else torch.gather(palette, 1, idx.reshape(f, -1, 1).expand(-1, -1, 3)).reshape(f, h, w, 3)
    return Q.compare(shown, frames)
