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
(``per_frame=True``).

True colour needs no palette: ``encode_jpeg`` turns the same frames into baseline JPEG streams where they are (``jpeg_coefficients``: colour transform, chroma
subsampling, an integer 8 x 8 DCT and the quantiser; ``jpeg_scan``: Huffman coding in restart intervals, byte stuffing), ``save_jpeg`` writes a still and
``save_avi`` a Motion-JPEG AVI, which needs no codec library to write and which ffmpeg, VLC and OpenCV read; ``read_avi`` takes one apart again.  The same
rule holds: p3d_video.h states every step in integers, the formulation here is the definition, the device bytes equal it.

Lossless needs no PIL either: ``encode_png`` makes every frame's zlib stream where the frames are (``png_filter``: the PNG row filters; ``png_counts``: the
symbol counts of run-length deflate per segment; ``png_deflate``: one length-limited Huffman code a frame, made on the host, and the bytes), ``save_png`` /
``save_png_sequence`` write stills, ``save_apng`` an animated PNG, and ``png_chunks`` takes a file apart again; 1 .. 4 bytes a pixel, palette indices and
16-bit grey (``depth16``) included.

What a setting costs is measured where the frames are (``quality.py``): ``jpeg_decode`` / ``jpeg_reconstruct`` show what a viewer of
the JPEGs sees without entropy decoding, ``jpeg_quality_for`` turns a PSNR or SSIM target into a quality (``encode_jpeg`` / ``save_avi`` take ``psnr=`` or
``ssim=`` in place of one), and ``palette_quality`` measures the GIF knobs.

The clips are read back where they are judged: ``jpeg_parse`` reads a baseline JPEG's header on the host, ``jpeg_unscan`` is the
entropy decoder — ``p3d_video_jpeg_unscan``, a lane per restart interval, with a status per interval for bytes that did not come from us — and
``decode_jpeg`` / ``load_jpeg`` / ``decode_avi`` put the two in front of ``jpeg_decode``; ``check_avi`` says whether a file shows what ``jpeg_reconstruct``
promised.  Our own streams and libjpeg's (optimised tables, any restart interval, grey) are served; progressive, 4:2:2 and 12-bit are refused by name."""
import collections

import numpy as np
import torch

from . import _lib

_side = _lib.SideLibrary('video')                    # libp3d_video.so: loaded on the first call, device-guarded; launch_count() is its own counter
VIDEO_LIB_PATH, HEADER = _side.path, _side.header
video_lib, launch_count, _check = _side.lib, _side.launch_count, _side.check
BINS, COLORS, MAX_AMPLITUDE = (HEADER.constants[k] for k in ('P3D_VIDEO_BINS', 'P3D_VIDEO_COLORS', 'P3D_VIDEO_MAX_AMPLITUDE'))
MAX_PIXELS = 1 << 31                                 # F * H * W stays below it


def _check_frames(frames, what='frames', bpp=(3,)):
    """(F, H, W) of uint8 [F, H, W, 3] frames with contiguous pixels and fewer than 2^31 of them; ValueError otherwise.  ``bpp``: the bytes a pixel may
    have — [F, H, W, bpp], and [F, H, W] for 1 — with fewer than 2^31 bytes (the PNG stages)."""
    shape = ' or '.join('[F, H, W]' if b == 1 else f'[F, H, W, {b}]' for b in bpp)
    ok = torch.is_tensor(frames) and frames.dtype == torch.uint8
    if not ok or not ((frames.ndim == 4 and frames.shape[3] in bpp and frames.shape[3] > 1) or (frames.ndim == 3 and 1 in bpp)):
        raise ValueError(f'{what} must be a uint8 {shape} tensor, got '
                         f'{str(frames.dtype) + " " + str(tuple(frames.shape)) if torch.is_tensor(frames) else type(frames).__name__}')
    f, h, w = frames.shape[:3]
    b = frames.shape[3] if frames.ndim == 4 else 1
    if f * h * w * (b if tuple(bpp) != (3,) else 1) >= MAX_PIXELS:
        raise ValueError(f'{what}: {f} x {h} x {w} pixels reach 2^31')
    strides = tuple(frames.stride()) + (1,) * (4 - frames.ndim)
    if f * h * w and (strides[3] != 1 or strides[2] != b or strides[1] < b * w or strides[0] < 0):
        raise ValueError(f'{what}: pixels must be contiguous (strides [*, >= {b * w}, {b}, 1]), got strides {tuple(frames.stride())}')
    return f, h, w


def _clip(frames):
    """The leading arguments of every entry point."""
    f, h, w = frames.shape[:3]
    return _lib.ptr(frames), frames.stride(0), frames.stride(1), f, h, w


def _bins(frames):
    v = frames.to(torch.int64) >> 3
    return (v[..., 0] << 10) | (v[..., 1] << 5) | v[..., 2]


# ---- histogram -------------------------------------------------------------------------------------------------------------------------
def histogram(frames, per_frame=False):
    """int32 [32768], or [F, 32768] with ``per_frame``: the number of pixels in every bin.  Device tensors: ``p3d_video_histogram`` (the histogram of a
    work-group in LDS, flushed with integer atomics); CPU tensors: ``bincount``."""
    f, h, w = _check_frames(frames)
    groups = f if per_frame else 1
    if f * h * w == 0:
        counts = torch.zeros([groups, BINS], dtype=torch.int32, device=frames.device)
    elif not frames.is_cuda:
        bins = _bins(frames).reshape(groups, -1)
        counts = torch.stack([torch.bincount(row, minlength=BINS) for row in bins]).to(torch.int32)
    else:
        counts = torch.empty([groups, BINS], dtype=torch.int32, device=frames.device)
        with _lib.kernel_timer('video_histogram', counts):
            code = video_lib().p3d_video_histogram(*_clip(frames), int(bool(per_frame)), _lib.ptr(counts), _lib.stream_of(counts))
        _check(code, 'video_histogram')
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
    f, h, w = _check_frames(frames)
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
            code = video_lib().p3d_video_box_sums(*_clip(frames), int(bool(per_frame)), _lib.ptr(lookup), _lib.ptr(sums), _lib.stream_of(sums))
        _check(code, 'video_box_sums')
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
    f, h, w = _check_frames(frames)
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
        code = video_lib().p3d_video_quantize(*_clip(frames), int(bool(per_frame)), _lib.ptr(full), _lib.ptr(n_colors), amplitude, _lib.ptr(out),
                                              out.stride(0), out.stride(1), _lib.stream_of(out))
    _check(code, 'video_quantize')
    return out


# ---- the four steps ------------------------------------------------------------------------------------------------------------------------
def palettize(frames, colors=COLORS, dither=0, palette='global'):
    """``(indices uint8 [F, H, W], palette uint8 [256, 3], n_colors int32 [1])`` for ``palette='global'`` — one palette for the clip, so flat areas do not
    shimmer from frame to frame — or ``(indices, palette [F, 256, 3], n_colors [F])`` for ``'frame'``, all on the frames' device.  The four steps: histogram,
    median cut to at most ``colors`` (2 .. 256) boxes, box means, nearest-row indices under the ordered dither of amplitude ``dither``.  Rows from
    ``n_colors`` on are zeros and never chosen.  The median cut runs on the host: the histogram (128 KB a group) is copied there and the lookup (32 KB a
    group) back — the ONLY synchronisation with the host; everything per pixel stays on the frames' device."""
    f, h, w = _check_frames(frames)
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


# ---- baseline JPEG and Motion-JPEG -----------------------------------------------------------------------------------------------------------
# True colour without a codec library: every frame a baseline JFIF of its own, the clip an AVI of them.  csrc/video/p3d_video.h states the rules; the
# formulations here are those rules operation by operation, and the kernels' bytes equal them.
JPEG_RESTART, JPEG_BLOCK_BITS = HEADER.constants['P3D_VIDEO_JPEG_RESTART'], HEADER.constants['P3D_VIDEO_JPEG_BLOCK_BITS']
MAX_AVI_BYTES = 1 << 31                              # a RIFF file of one 'movi' list stays below it (OpenDML is out of scope)
_SUBSAMPLING = {'4:4:4': 0, '4:2:0': 1}
_BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# Annex K.3: (BITS: the number of codes of every length 1 .. 16, HUFFVAL: the symbols in code order) of DC luma, DC chroma, AC luma, AC chroma.
_AC_LUMA_VALUES = bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a53545556'
    '5758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6'
    'd7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa')
_AC_CHROMA_VALUES = bytes.fromhex(
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a5354'
    '55565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3'
    'd4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa')
_ANNEX_K = (((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
            ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
            ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), tuple(_AC_LUMA_VALUES)),
            ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), tuple(_AC_CHROMA_VALUES)))


def jpeg_zigzag():
    """int64 [64]: the natural index 8 v + u of every zigzag position — the diagonals v + u in turn, odd ones downwards (v rising), even ones upwards."""
    return torch.tensor(sorted(range(64), key=lambda n: (n // 8 + n % 8, n // 8 if (n // 8 + n % 8) % 2 else n % 8)), dtype=torch.int64)


def jpeg_dct_table():
    """int64 [8, 8]: T[u][x] = round(8192 a(u) cos((2 x + 1) u pi / 16)), a(0) = sqrt(1 / 8), a(u) = 1 / 2 otherwise — the literals of p3d_video.h."""
    u, x = np.arange(8.0)[:, None], np.arange(8.0)[None, :]
    a = np.where(u == 0, np.sqrt(0.125), 0.5)
    return torch.from_numpy(np.round(8192 * a * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64))


def jpeg_dct(samples):
    """int64 [..., 8, 8] (v, u) of integer level-shifted samples [..., 8, 8] (y, x): 8 x the orthonormal DCT by the header's two integer passes,
    r[y][u] = (sum_x T[u][x] s[y][x] + 128) >> 8, then c8[v][u] = (sum_y T[v][y] r[y][u] + 16384) >> 15, with arithmetic shifts."""
    t = jpeg_dct_table()
    r = (torch.matmul(samples.to(torch.int64), t.T) + 128) >> 8
    return (torch.matmul(t, r) + 16384) >> 15


def _check_quality(quality):
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError(f'quality must be an integer 1 .. 100, got {quality!r}')
    return int(quality)


def jpeg_tables(quality):
    """(luma, chroma): two uint8 [64] quantisation tables in ZIGZAG order on the host — the Annex K base tables under the IJG scaling, scale = 5000 / quality
    (an integer division) below 50 and 200 - 2 quality from 50, entry = clamp((base scale + 50) / 100, 1, 255).  1 <= ``quality`` <= 100."""
    q = _check_quality(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    zigzag = jpeg_zigzag()
    return tuple(((torch.tensor(base, dtype=torch.int64) * scale + 50) // 100).clamp(1, 255).to(torch.uint8)[zigzag] for base in (_BASE_LUMA, _BASE_CHROMA))


class JpegHuffman:
    """The four Annex K tables, in the order DC luma, DC chroma, AC luma, AC chroma: ``bits`` (four tuples of 16: the number of codes of every length) and
    ``values`` (four tuples: the symbols in code order) as a DHT segment states them, and ``lookup`` uint32 [4, 256] on the host: per table and symbol
    length << 16 | code, 0 for a symbol without a code — what ``p3d_video_jpeg_scan`` reads."""

    def __init__(self):
        self.bits, self.values = tuple(b for b, _ in _ANNEX_K), tuple(v for _, v in _ANNEX_K)
        lookup = np.zeros([4, 256], dtype=np.int64)
        for t, (bits, values) in enumerate(_ANNEX_K):
            code, k = 0, 0
            for length, n in enumerate(bits, start=1):                          # the canonical assignment of Annex C
                for _ in range(n):
                    lookup[t, values[k]] = length << 16 | code
                    code, k = code + 1, k + 1
                code <<= 1
        self.lookup = torch.from_numpy(lookup.astype(np.uint32).view(np.int32)).view(torch.int32)      # (torch has little use for uint32: the same 32 bits)


_huffman = None
_on_device = {}                                      # (what, device) -> the constant tables there: uploaded once


def jpeg_huffman():
    """The ``JpegHuffman`` of this module (made once)."""
    global _huffman
    if _huffman is None:
        _huffman = JpegHuffman()
    return _huffman


def _device_tables(what, device, make):
    key = (what, str(device))
    if key not in _on_device:
        _on_device[key] = tuple(t.to(device) for t in make())
    return _on_device[key]


def _check_subsampling(subsampling):
    if subsampling in (0, 1) and not isinstance(subsampling, bool):
        return int(subsampling)
    if subsampling not in _SUBSAMPLING:
        raise ValueError(f"subsampling must be '4:4:4' or '4:2:0' (0 or 1), got {subsampling!r}")
    return _SUBSAMPLING[subsampling]


def jpeg_layout(h, w, subsampling):
    """(MCUs of a row, MCUs of a frame, blocks of an MCU, restart intervals of a frame) of an ``h`` x ``w`` picture."""
    sub = _check_subsampling(subsampling)
    mcu = 8 << sub
    mcus_x, mcus_y = -(-int(w) // mcu), -(-int(h) // mcu)
    return mcus_x, mcus_x * mcus_y, 6 if sub else 3, -(-(mcus_x * mcus_y) // JPEG_RESTART)


def _jpeg_coefficients_torch(frames, luma_q, chroma_q, sub):
    f, h, w = frames.shape[:3]
    mcu = 8 << sub
    hp, wp = -(-h // mcu) * mcu, -(-w // mcu) * mcu
    rows, cols = torch.arange(hp).clamp(max=h - 1), torch.arange(wp).clamp(max=w - 1)      # the last row and column repeat
    rgb = frames[:, rows][:, :, cols].to(torch.int64)
    r, g, b = rgb.unbind(dim=3)
    planes = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
              ((-11059 * r - 21709 * g + 32768 * b + 32768 + (128 << 16)) >> 16).clamp(0, 255),
              ((32768 * r - 27439 * g - 5329 * b + 32768 + (128 << 16)) >> 16).clamp(0, 255)]
    if sub:
        planes[1:] = [(p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2] + 2) >> 2 for p in planes[1:]]
    zigzag = jpeg_zigzag()

    def blocks(plane, q):
        """[F, rows of blocks, columns of blocks, 64]: the quantised coefficients of every 8 x 8 block in zigzag order."""
        hb, wb = plane.shape[1] // 8, plane.shape[2] // 8
        c8 = jpeg_dct(plane.reshape(f, hb, 8, wb, 8).permute(0, 1, 3, 2, 4) - 128).reshape(f, hb, wb, 64)[..., zigzag]
        q = q.to(torch.int64).clamp(min=1)
        return torch.sign(c8) * ((c8.abs() + 4 * q) // (8 * q))
    y, cb, cr = blocks(planes[0], luma_q), blocks(planes[1], chroma_q), blocks(planes[2], chroma_q)
    my, mx = hp // mcu, wp // mcu
    if sub:                                                                       # Y00 Y01 Y10 Y11 of every MCU
        y = y.reshape(f, my, 2, mx, 2, 64).permute(0, 1, 3, 2, 4, 5).reshape(f, my, mx, 4, 64)
    else:
        y = y[:, :, :, None]
    return torch.cat([y, cb[:, :, :, None], cr[:, :, :, None]], dim=3).reshape(f, my * mx, -1, 64).to(torch.int16)


def jpeg_coefficients(frames, tables, subsampling='4:2:0'):
    """int16 [F, n_mcu, 3 or 6, 64]: the quantised DCT coefficients of the frames, MCUs in raster order, the blocks of an MCU Y Cb Cr (4:4:4, an MCU of
    8 x 8 pixels) or Y00 Y01 Y10 Y11 Cb Cr (4:2:0, 16 x 16), every block in zigzag order.  ``tables``: (luma, chroma) uint8 [64] in zigzag order
    (``jpeg_tables``).  The rules — the fixed-point JFIF colour transform, edge replication up to the MCU, the rounded 2 x 2 chroma mean, the two integer DCT
    passes, the rounding quantiser — are p3d_video.h's.  Device tensors: ONE ``p3d_video_jpeg_blocks`` launch; CPU tensors: the torch formulation."""
    f, h, w = _check_frames(frames)
    sub = _check_subsampling(subsampling)
    luma_q, chroma_q = (torch.as_tensor(t) for t in tables)
    for t in (luma_q, chroma_q):
        if t.dtype != torch.uint8 or tuple(t.shape) != (64,):
            raise ValueError('jpeg_coefficients: tables must be two uint8 [64] tensors')
    _, n_mcu, bpm, _ = jpeg_layout(h, w, sub)
    if f * h * w == 0:
        return torch.zeros([f, 0, bpm, 64], dtype=torch.int16, device=frames.device)      # no pixel, no MCU
    if not frames.is_cuda:
        return _jpeg_coefficients_torch(frames, luma_q.cpu(), chroma_q.cpu(), sub)
    luma_q, chroma_q = luma_q.to(frames.device).contiguous(), chroma_q.to(frames.device).contiguous()
    out = torch.empty([f, n_mcu, bpm, 64], dtype=torch.int16, device=frames.device)
    with _lib.kernel_timer('video_jpeg_blocks', out):
        code = video_lib().p3d_video_jpeg_blocks(*_clip(frames), sub, _lib.ptr(luma_q), _lib.ptr(chroma_q), _lib.ptr(out), _lib.stream_of(out))
    _check(code, 'video_jpeg_blocks')
    return out


def _bit_length(v):
    """The size category of every entry: the number of bits of its magnitude (0 for 0; the entries stay below 2^11)."""
    a = np.abs(v)
    return sum(((a >> b) > 0).astype(np.int64) for b in range(11))


def _jpeg_scan_numpy(blocks, bpm):
    """The scan bytes of ONE frame: ``blocks`` int64 [n_mcu * bpm, 64].  Every (block, coefficient) slot and every block's end becomes a token of up to 59 bits
    (the ZRLs before a value, its code, its extra bits); the tokens' bit positions are a cumulative sum that restarts, byte-aligned, at every interval."""
    table = jpeg_huffman().lookup.numpy().view(np.uint32).astype(np.int64)
    code, length = table & 0xFFFF, table >> 16
    nb = blocks.shape[0]
    k = np.arange(nb) % bpm
    interval = np.arange(nb) // bpm // JPEG_RESTART
    n_intervals = int(interval[-1]) + 1
    component = k if bpm == 3 else np.maximum(k - 3, 0)
    chroma = (component > 0).astype(np.int64)
    dc, ac = np.clip(blocks[:, 0], -1024, 1023), np.clip(blocks[:, 1:], -1023, 1023)
    pred = np.zeros(nb, dtype=np.int64)
    for c in range(3):                                                            # the previous block of the same component, if the interval holds it
        idx = np.flatnonzero(component == c)
        pred[idx[1:]] = np.where(interval[idx[1:]] == interval[idx[:-1]], dc[idx[:-1]], 0)
    values, lengths = np.zeros([nb, 65], dtype=np.int64), np.zeros([nb, 65], dtype=np.int64)

    def extra(v, size):
        return np.where(v < 0, v - 1, v) & ((1 << size) - 1)
    d = dc - pred
    size = _bit_length(d)
    values[:, 0], lengths[:, 0] = code[chroma, size] << size | extra(d, size), length[chroma, size] + size
    position = np.arange(1, 64)[None, :]
    nonzero = ac != 0
    before = np.maximum.accumulate(np.where(nonzero, position, 0), axis=1)        # the last non-zero position up to here ...
    before = np.concatenate([np.zeros([nb, 1], dtype=np.int64), before[:, :-1]], axis=1)      # ... and before here (0: the DC)
    run = position - before - 1
    size = _bit_length(ac)
    tab = (2 + chroma)[:, None]
    v, n = code[tab, (run & 15) << 4 | size] << size | extra(ac, size), length[tab, (run & 15) << 4 | size] + size
    for j in range(3):                                                            # one ZRL per 16 zeros of the run, in front
        more = (run >> 4) > j
        v, n = np.where(more, code[tab, 0xF0] << n | v, v), np.where(more, n + length[tab, 0xF0], n)
    values[:, 1:64], lengths[:, 1:64] = np.where(nonzero, v, 0), np.where(nonzero, n, 0)
    values[:, 64], lengths[:, 64] = code[2 + chroma, 0], np.where(ac[:, 62] == 0, length[2 + chroma, 0], 0)      # EOB unless coefficient 63 is non-zero

    values, lengths, token_interval = values.reshape(-1), lengths.reshape(-1), np.repeat(interval, 65)
    first = np.cumsum(lengths) - lengths
    interval_bits = np.bincount(token_interval, weights=lengths, minlength=n_intervals).astype(np.int64)
    interval_bytes = (interval_bits + 7) // 8
    base = np.cumsum(interval_bytes) - interval_bytes                              # of an interval, in the unstuffed bytes
    first = first - (np.cumsum(interval_bits) - interval_bits)[token_interval] + 8 * base[token_interval]
    bits = np.zeros(8 * int(interval_bytes.sum()), dtype=np.uint8)
    for b in range(int(lengths.max())):
        on = lengths > b
        bits[first[on] + b] = (values[on] >> (lengths[on] - 1 - b)) & 1
    for b in range(7):                                                            # 1-bits up to the byte
        on = interval_bits + b < 8 * interval_bytes
        bits[8 * base[on] + interval_bits[on] + b] = 1
    raw = np.packbits(bits)
    ff = (raw == 255).astype(np.int64)
    stuffed_before = np.cumsum(ff) - ff
    place = np.arange(raw.shape[0]) + stuffed_before + 2 * np.repeat(np.arange(n_intervals), interval_bytes)
    out = np.zeros(raw.shape[0] + int(ff.sum()) + 2 * (n_intervals - 1), dtype=np.uint8)
    out[place] = raw
    marked = np.arange(n_intervals - 1)                                           # every interval but the last: RSTm after it
    at = base[1:] + np.cumsum(ff)[base[1:] - 1] + 2 * marked
    out[at], out[at + 1] = 255, 0xD0 + (marked & 7)
    return out


def jpeg_scan(coefficients, h, w, subsampling='4:2:0'):
    """``(data uint8 [total], offsets int64 [F + 1])``: the entropy-coded scans of ``coefficients`` (``jpeg_coefficients``' layout, for pictures of ``h`` x ``w``),
    frame i at ``data[offsets[i]:offsets[i + 1]]``; ``data`` on the coefficients' device, ``offsets`` on the host.  A frame is cut into restart intervals of
    ``JPEG_RESTART`` MCUs: each starts byte-aligned with the DC predictors 0, is padded with 1-bits, byte-stuffed and — but for the last — followed by RSTm,
    m = interval index mod 8, so that no interval shares a bit with another.  The Annex K tables (``jpeg_huffman``).  Device tensors: two
    ``p3d_video_jpeg_scan`` launches — the byte length of every interval, then, after their prefix sum, the bytes — with the copy of the lengths to the
    host between them, the ONLY synchronisation (it sizes ``data``).  CPU tensors: the numpy formulation, frame by frame."""
    sub = _check_subsampling(subsampling)
    _, n_mcu, bpm, n_intervals = jpeg_layout(h, w, sub)
    if not torch.is_tensor(coefficients) or coefficients.dtype != torch.int16 or coefficients.ndim != 4:
        raise ValueError('jpeg_scan: coefficients must be an int16 [F, n_mcu, blocks, 64] tensor')
    f = coefficients.shape[0]
    if int(h) < 0 or int(w) < 0 or f * int(h) * int(w) >= MAX_PIXELS:
        raise ValueError(f'jpeg_scan: {f} x {h} x {w} pixels are negative or reach 2^31')
    if f * int(h) * int(w) == 0:
        return torch.zeros([0], dtype=torch.uint8, device=coefficients.device), torch.zeros([f + 1], dtype=torch.int64)
    if tuple(coefficients.shape[1:]) != (n_mcu, bpm, 64):
        raise ValueError(f'jpeg_scan: {h} x {w} at subsampling {subsampling!r} has [{n_mcu}, {bpm}, 64] coefficients a frame, got {list(coefficients.shape[1:])}')
    if not coefficients.is_cuda:
        scans = [_jpeg_scan_numpy(c.reshape(-1, 64).to(torch.int64).numpy(), bpm) for c in coefficients]
        sizes = torch.tensor([0] + [s.shape[0] for s in scans], dtype=torch.int64)
        return torch.from_numpy(np.concatenate(scans)), torch.cumsum(sizes, 0)
    coefficients = coefficients.contiguous()
    huffman, = _device_tables('huffman', coefficients.device, lambda: (jpeg_huffman().lookup,))
    lengths = torch.empty([f, n_intervals], dtype=torch.int32, device=coefficients.device)
    stream = lambda: _lib.stream_of(coefficients)
    with _lib.kernel_timer('video_jpeg_scan_lengths', lengths):
        code = video_lib().p3d_video_jpeg_scan(_lib.ptr(coefficients), f, int(h), int(w), sub, _lib.ptr(huffman), _lib.ptr(lengths), None, None, 0, stream())
    _check(code, 'video_jpeg_scan')
    ends = torch.cumsum(lengths.reshape(-1), 0, dtype=torch.int64)
    starts = ends - lengths.reshape(-1)                                            # on the device: the second launch does not wait for the host
    offsets = torch.cat([torch.zeros([1], dtype=torch.int64), torch.cumsum(lengths.cpu().sum(dim=1, dtype=torch.int64), 0)])
    data = torch.empty([int(offsets[-1])], dtype=torch.uint8, device=coefficients.device)
    with _lib.kernel_timer('video_jpeg_scan_bytes', data):
        code = video_lib().p3d_video_jpeg_scan(_lib.ptr(coefficients), f, int(h), int(w), sub, _lib.ptr(huffman), None, _lib.ptr(starts), _lib.ptr(data),
                                               data.shape[0], stream())
    _check(code, 'video_jpeg_scan')
    return data, offsets


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + payload


def jpeg_header(h, w, tables, subsampling='4:2:0'):
    """Everything of a baseline JFIF before its scan: SOI, APP0 (JFIF 1.01, square pixels), two DQT, SOF0 (8 bits, three components, Y sampled 2 x 2 at 4:2:0),
    the four Annex K DHT, DRI (``JPEG_RESTART`` MCUs) and SOS.  The scan and EOI (0xFF 0xD9) follow."""
    sub = _check_subsampling(subsampling)
    if not (1 <= int(h) <= 65535 and 1 <= int(w) <= 65535):
        raise ValueError(f'a JPEG is 1 .. 65535 pixels a side, got {h} x {w}')
    huffman = jpeg_huffman()
    out = b'\xff\xd8' + _segment(0xE0, b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, table in enumerate(tables):
        out += _segment(0xDB, bytes([i]) + bytes(torch.as_tensor(table).cpu().tolist()))
    out += _segment(0xC0, bytes([8]) + int(h).to_bytes(2, 'big') + int(w).to_bytes(2, 'big') + bytes([3, 1, 0x22 if sub else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for i, (bits, values) in enumerate(zip(huffman.bits, huffman.values)):       # Tc << 4 | Th: DC 0, DC 1, AC 0, AC 1
        out += _segment(0xC4, bytes([(i >> 1) << 4 | (i & 1)]) + bytes(bits) + bytes(values))
    out += _segment(0xDD, JPEG_RESTART.to_bytes(2, 'big'))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode_jpeg(frames, quality=90, subsampling='4:2:0', psnr=None, ssim=None):
    """A list of ``bytes``, one complete baseline JFIF per frame of uint8 [F, H, W, 3] (the module's frame contract; on the device or the host, or a numpy
    array): ``jpeg_header``, the frame's scan, EOI.  ``quality`` 1 .. 100 picks the tables (``jpeg_tables``).  From device frames: the two kernels' three
    launches, ONE synchronisation with the host (the interval lengths) and ONE device -> host copy (the scans, a few percent of the frames' bytes).
    ``psnr`` or ``ssim`` (ONE of them): a target instead of a setting — ``jpeg_quality_for`` picks the quality, ``quality`` plays no part, and the tables in
    the streams (``jpeg_tables`` of the choice) say what it was."""
    frames = torch.as_tensor(frames)
    f, h, w = _check_frames(frames)
    if psnr is not None or ssim is not None:
        _check_target(psnr, ssim, 'encode_jpeg')
        if f * h * w:
            quality = jpeg_quality_for(frames, psnr, ssim, subsampling)[0]
    sub, tables = _check_subsampling(subsampling), jpeg_tables(quality)
    if f == 0:
        return []
    header = jpeg_header(h, w, tables, sub)
    on_device = _device_tables(('quantisation', _check_quality(quality)), frames.device, lambda: tables) if frames.is_cuda else tables
    data, offsets = jpeg_scan(jpeg_coefficients(frames, on_device, sub), h, w, sub)
    data, offsets = data.cpu().numpy().tobytes(), offsets.tolist()
    return [header + data[offsets[i]:offsets[i + 1]] + b'\xff\xd9' for i in range(f)]


def save_jpeg(path, frame, quality=90, subsampling='4:2:0'):
    """One uint8 [H, W, 3] frame, on the device or the host, as a baseline JPEG file (``encode_jpeg``).  Returns its bytes."""
    frame = torch.as_tensor(frame)
    if frame.ndim != 3:
        raise ValueError(f'save_jpeg: frame must be uint8 [H, W, 3], got {tuple(frame.shape)}')
    stream, = encode_jpeg(frame[None], quality, subsampling)
    with open(path, 'wb') as fh:
        fh.write(stream)
    return stream


def _chunk(fourcc, payload):
    return fourcc + len(payload).to_bytes(4, 'little') + payload + b'\0' * (len(payload) & 1)


def save_avi(path, frames, fps=60, quality=90, subsampling='4:2:0', psnr=None, ssim=None):
    """The frames (``encode_jpeg``'s contract) as a Motion-JPEG AVI: a RIFF 'AVI ' file with the list 'hdrl' ('avih', and one 'strl' of 'strh' — 'vids' /
    'MJPG', the rate ``fps`` as dwRate / dwScale — and 'strf', a 40-byte BITMAPINFOHEADER of 24 bits), the list 'movi' of one '00dc' chunk per frame,
    padded to an even length, and 'idx1': per frame the key-frame flag, the chunk's offset from 'movi' and its length.  Every frame is a key frame.
    ValueError for no frame and for a file that would reach 2^31 bytes (OpenDML is out of scope).  ``psnr`` / ``ssim``: ``encode_jpeg``'s target, which
    then picks the quality.  Returns the JPEG streams."""
    import fractions
    import struct
    frames = torch.as_tensor(frames)
    f, h, w = _check_frames(frames)
    if f == 0:
        raise ValueError('save_avi: an AVI needs at least one frame')
    rate = fractions.Fraction(fps).limit_denominator(1 << 16)
    if rate <= 0:
        raise ValueError(f'save_avi: fps must be > 0, got {fps!r}')
    streams = encode_jpeg(frames, quality, subsampling, psnr, ssim)
    movi, index = b'movi', b''
    chunks = [movi]
    at = 4                                                                        # of the next chunk, from the 'movi' word
    for s in streams:
        index += b'00dc' + struct.pack('<III', 0x10, at, len(s))                  # AVIIF_KEYFRAME
        chunks.append(_chunk(b'00dc', s))
        at += len(chunks[-1])
    largest = max(len(s) for s in streams)
    avih = struct.pack('<14I', round(1e6 / rate), int(largest * rate) + 1, 0, 0x10, f, 0, 1, largest, w, h, 0, 0, 0, 0)       # AVIF_HASINDEX
    strh = b'vidsMJPG' + struct.pack('<IHHIIIIIIIi4H', 0, 0, 0, 0, rate.denominator, rate.numerator, 0, f, largest, 0xFFFFFFFF, 0, 0, 0, w, h)
    strf = struct.pack('<IiiHH4sIiiII', 40, w, h, 1, 24, b'MJPG', 3 * w * h, 0, 0, 0, 0)
    hdrl = b'hdrl' + _chunk(b'avih', avih) + _chunk(b'LIST', b'strl' + _chunk(b'strh', strh) + _chunk(b'strf', strf))
    body = b'AVI ' + _chunk(b'LIST', hdrl) + _chunk(b'LIST', b''.join(chunks)) + _chunk(b'idx1', index)
    if len(body) + 8 >= MAX_AVI_BYTES:
        raise ValueError(f'save_avi: the file would take {len(body) + 8} bytes; an AVI of one RIFF chunk stays below 2^31')
    with open(path, 'wb') as fh:
        fh.write(b'RIFF' + len(body).to_bytes(4, 'little') + body)
    return streams


def read_avi(path):
    """``(the JPEG bytes of every frame, fps, (w, h))`` of a Motion-JPEG AVI, by following 'idx1' into 'movi' — for tests, and for users without a player.
    ``fps`` is dwRate / dwScale of the stream header, an int where that is whole.  ValueError for anything that is not such a file."""
    import struct
    with open(path, 'rb') as fh:
        data = fh.read()
    if len(data) < 12 or data[:4] != b'RIFF' or data[8:12] != b'AVI ':
        raise ValueError(f'read_avi: {path} is not a RIFF AVI file')

    def chunks(begin, end):
        """(fourcc, payload begin, payload end) of the chunks in data[begin:end]; of a LIST the fourcc is its type and the payload what follows it."""
        while begin + 8 <= end:
            fourcc, size = data[begin:begin + 4], int.from_bytes(data[begin + 4:begin + 8], 'little')
            if begin + 8 + size > end:
                raise ValueError(f'read_avi: the chunk {fourcc!r} at {begin} runs past its parent')
            yield (data[begin + 8:begin + 12], begin + 12, begin + 8 + size) if fourcc == b'LIST' else (fourcc, begin + 8, begin + 8 + size)
            begin += 8 + size + (size & 1)
    top = {name: (a, b) for name, a, b in chunks(12, min(len(data), 8 + int.from_bytes(data[4:8], 'little')))}
    if not all(name in top for name in (b'hdrl', b'movi', b'idx1')):
        raise ValueError(f'read_avi: {path} lacks one of hdrl, movi, idx1')
    strl = {name: (a, b) for name, a, b in chunks(*dict((n, (a, b)) for n, a, b in chunks(*top[b'hdrl']))[b'strl'])}
    strh, strf = data[slice(*strl[b'strh'])], data[slice(*strl[b'strf'])]
    if strh[:8] != b'vidsMJPG':
        raise ValueError(f'read_avi: the stream is {strh[:8]!r}, not vids / MJPG')
    scale, rate = struct.unpack('<II', strh[20:28])
    w, h = struct.unpack('<ii', strf[4:12])
    movi = top[b'movi'][0] - 4                                                     # the 'movi' word: what idx1 counts from
    streams = []
    for entry in range(top[b'idx1'][0], top[b'idx1'][1], 16):
        fourcc, _, offset, size = struct.unpack('<4sIII', data[entry:entry + 16])
        at = movi + offset
        if fourcc != b'00dc' or data[at:at + 4] != b'00dc' or int.from_bytes(data[at + 4:at + 8], 'little') != size:
            raise ValueError(f'read_avi: the index entry at {entry} does not point at a 00dc chunk of {size} bytes')
        streams.append(data[at + 8:at + 8 + size])
    return streams, (rate // scale if rate % scale == 0 else rate / scale), (w, h)


# ---- the way back: what a setting costs ------------------------------------------------------------------------------------------------------
# A decoder's view of the coefficients without entropy decoding, so that ``quality.compare`` can judge a setting where the frames are, and the search
# that turns a target into a setting.
def jpeg_idct(coefficients):
    """int64 [..., 8, 8] (y, x) of dequantised coefficients [..., 8, 8] (v, u) in natural order: the header's two integer passes, the column pass
    m[y][u] = (sum_v T[v][y] c[v][u] + 512) >> 10, then the row pass s[y][x] = (sum_u T[u][x] m[y][u] + 32768) >> 16 — the level-shifted sample."""
    t = jpeg_dct_table()
    m = (torch.matmul(t.T, coefficients.to(torch.int64)) + 512) >> 10
    return (torch.matmul(m, t) + 32768) >> 16


def jpeg_dequantize(coefficients, tables, subsampling):
    """int64 [F, n_mcu, blocks, 8, 8] (v, u): ``jpeg_coefficients``' int16 blocks times their table's entries (a 0 counts as 1), clamped to int16's range and
    taken out of zigzag order."""
    sub = _check_subsampling(subsampling)
    luma_q, chroma_q = (torch.as_tensor(t).cpu().to(torch.int64).clamp(min=1) for t in tables)
    n_luma = 4 if sub else 1
    q = torch.stack([luma_q] * n_luma + [chroma_q] * 2)                            # [blocks, 64]
    c = (coefficients.to(torch.int64) * q).clamp(-32768, 32767)
    natural = torch.empty_like(c)
    natural[..., jpeg_zigzag()] = c
    return natural.reshape(*c.shape[:-1], 8, 8)


def _jpeg_decode_torch(coefficients, tables, h, w, sub, out):
    f = coefficients.shape[0]
    mcu = 8 << sub
    my, mx = -(-h // mcu), -(-w // mcu)
    s = (jpeg_idct(jpeg_dequantize(coefficients, tables, sub)) + 128).clamp(0, 255).reshape(f, my, mx, -1, 8, 8)

    def plane(blocks):                                                            # [F, my, mx, 8, 8] -> [F, 8 my, 8 mx]
        return blocks.permute(0, 1, 3, 2, 4).reshape(f, my * 8, mx * 8)
    if sub:
        y = s[:, :, :, :4].reshape(f, my, mx, 2, 2, 8, 8).permute(0, 1, 3, 5, 2, 4, 6).reshape(f, my * 16, mx * 16)
        ch, cw = (h + 1) // 2, (w + 1) // 2
        rows, cols = torch.arange(h), torch.arange(w)
        near, cx = rows >> 1, cols >> 1
        far = (near + torch.where(rows & 1 == 1, 1, -1)).clamp(0, ch - 1)
        ox = (cx + torch.where(cols & 1 == 1, 1, -1)).clamp(0, cw - 1)
        bias = torch.where(cols & 1 == 1, 7, 8)
        chroma = []
        for k in (4, 5):
            p = plane(s[:, :, :, k])[:, :ch, :cw]
            v = 3 * p[:, near] + p[:, far]                                        # [F, h, cw]
            chroma.append((3 * v[:, :, cx] + v[:, :, ox] + bias) >> 4)
        cb, cr = chroma
    else:
        y, cb, cr = (plane(s[:, :, :, k]) for k in range(3))
    y, cb, cr = y[:, :h, :w], cb[:, :h, :w] - 128, cr[:, :h, :w] - 128
    rgb = torch.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], dim=3)
    out.copy_(rgb.clamp(0, 255).to(torch.uint8))
    return out


def jpeg_decode(coefficients, tables, h, w, subsampling='4:2:0', out=None):
    """uint8 [F, h, w, 3]: what a decoder shows for ``coefficients`` (``jpeg_coefficients``' layout, for pictures of ``h`` x ``w``) under ``tables`` — no
    entropy decoding, so a quality setting is judged where the frames are.  p3d_video.h states the rules: dequantise and clamp to int16, the inverse of
    the integer DCT in two passes with 26 bits of rounding shifts, + 128 and clamp; at 4:2:0 the triangle filter on the chroma planes (3 : 1 vertically,
    then 3 : 1 horizontally with the roundings 8 and 7, edges replicated); the fixed-point JFIF inverse colour transform; the crop.  Not bit-equal with any
    libjpeg (their inverse DCTs differ by a level here and there), but the same picture.  ``out``: the caller's uint8 [F, h, w, 3] view with contiguous
    pixels and any pitches.  Device tensors: TWO launches of ``p3d_video_jpeg_decode`` (blocks into planes in a scratch buffer, then pixels), no
    synchronisation; CPU tensors: the torch formulation."""
    sub = _check_subsampling(subsampling)
    h, w = int(h), int(w)
    _, n_mcu, bpm, _ = jpeg_layout(h, w, sub)
    if not torch.is_tensor(coefficients) or coefficients.dtype != torch.int16 or coefficients.ndim != 4:
        raise ValueError('jpeg_decode: coefficients must be an int16 [F, n_mcu, blocks, 64] tensor')
    f = coefficients.shape[0]
    if h < 0 or w < 0 or f * h * w >= MAX_PIXELS:
        raise ValueError(f'jpeg_decode: {f} x {h} x {w} pixels are negative or reach 2^31')
    luma_q, chroma_q = (torch.as_tensor(t) for t in tables)
    for t in (luma_q, chroma_q):
        if t.dtype != torch.uint8 or tuple(t.shape) != (64,):
            raise ValueError('jpeg_decode: tables must be two uint8 [64] tensors')
    if out is None:
        out = torch.empty([f, h, w, 3], dtype=torch.uint8, device=coefficients.device)
    elif not torch.is_tensor(out) or tuple(out.shape) != (f, h, w, 3) or out.device != coefficients.device:
        raise ValueError(f'jpeg_decode: out must be uint8 [{f}, {h}, {w}, 3] on {coefficients.device}')
    else:
        _check_frames(out, 'jpeg_decode: out')
        if f > 1 and h * w and out.stride(0) < h * out.stride(1):
            raise ValueError(f'jpeg_decode: the frames of out overlap (strides {tuple(out.stride())})')
    if f * h * w == 0:
        return out
    if tuple(coefficients.shape[1:]) != (n_mcu, bpm, 64):
        raise ValueError(f'jpeg_decode: {h} x {w} at subsampling {subsampling!r} has [{n_mcu}, {bpm}, 64] coefficients a frame, got {list(coefficients.shape[1:])}')
    if not coefficients.is_cuda:
        return _jpeg_decode_torch(coefficients, (luma_q, chroma_q), h, w, sub, out)
    coefficients = coefficients.contiguous()
    luma_q, chroma_q = luma_q.to(coefficients.device).contiguous(), chroma_q.to(coefficients.device).contiguous()
    mcu = 8 << sub
    plane = (-(-h // mcu) * mcu) * (-(-w // mcu) * mcu)
    scratch = torch.empty([f * (plane + 2 * (plane >> (2 * sub)))], dtype=torch.uint8, device=coefficients.device)
    with _lib.kernel_timer('video_jpeg_decode', out):
        code = video_lib().p3d_video_jpeg_decode(_lib.ptr(coefficients), f, h, w, sub, _lib.ptr(luma_q), _lib.ptr(chroma_q), _lib.ptr(scratch), scratch.shape[0],
                                                 _lib.ptr(out), out.stride(0), out.stride(1), _lib.stream_of(out))
    _check(code, 'video_jpeg_decode')
    return out


def jpeg_reconstruct(frames, quality=90, subsampling='4:2:0'):
    """uint8 [F, H, W, 3] on the frames' device: what a viewer of ``encode_jpeg(frames, quality, subsampling)`` sees — ``jpeg_decode`` of ``jpeg_coefficients``,
    three launches and no synchronisation from device frames."""
    frames = torch.as_tensor(frames)
    f, h, w = _check_frames(frames)
    sub, tables = _check_subsampling(subsampling), jpeg_tables(quality)
    if frames.is_cuda:
        tables = _device_tables(('quantisation', _check_quality(quality)), frames.device, lambda: tables)
    return jpeg_decode(jpeg_coefficients(frames, tables, sub), tables, h, w, sub)


def _check_target(psnr, ssim, what):
    """('psnr' or 'ssim', the target): exactly ONE of the two is given.  Both would need a rule for a quality that meets one and not the other; a caller who
    wants both takes the larger of two searches."""
    if (psnr is None) == (ssim is None):
        raise ValueError(f'{what}: give psnr (dB) or ssim (0 .. 1), one of them, got psnr={psnr!r}, ssim={ssim!r}')
    key, target = ('psnr', psnr) if ssim is None else ('ssim', ssim)
    if isinstance(target, bool) or not isinstance(target, (int, float)) or target != target or (key == 'ssim' and not 0 <= target <= 1) or (key == 'psnr' and target < 0):
        raise ValueError(f'{what}: {key} must be a number{" 0 .. 1" if key == "ssim" else " >= 0 (dB)"}, got {target!r}')
    return key, float(target)


def jpeg_quality_for(frames, psnr=None, ssim=None, subsampling='4:2:0', sample=8):
    """``(quality, metrics, met)``: the JPEG quality that meets a target — ``psnr`` in dB or ``ssim`` in 0 .. 1, ONE of them (``_check_target``) — as
    ``quality.compare`` measures ``jpeg_reconstruct`` against the frames, on at most ``sample`` evenly spaced frames of the clip (the first and the last among
    them).  A bisection of 1 .. 100 in at most seven steps, each three launches for the reconstruction, two for the sums and ONE host read.  The measure
    need not rise with the quality, so the promise is a post-condition, ``mesh.simplify_to``'s: the quality returned met the target as measured (``metrics``
    is its ``compare`` dict), and the quality below it was tried and did not (unless it is 1); if 100 does not meet it, ``(100, its metrics, False)``.  A
    clip without a sample — or, for ``ssim``, without a window — measures NaN, which meets nothing."""
    from . import quality as Q
    frames = torch.as_tensor(frames)
    f, h, w = _check_frames(frames)
    key, target = _check_target(psnr, ssim, 'jpeg_quality_for')
    sub = _check_subsampling(subsampling)
    if isinstance(sample, bool) or int(sample) != sample or int(sample) < 1:
        raise ValueError(f'jpeg_quality_for: sample must be an integer >= 1, got {sample!r}')
    n = int(sample)
    if f > n:
        frames = frames[[0] if n == 1 else [(i * (f - 1)) // (n - 1) for i in range(n)]]
    measured = {}
    low, high = 1, 101                                                            # the answer lies in low .. high; 101: none
    while low < high:
        mid = (low + high) // 2
        measured[mid] = Q.compare(jpeg_reconstruct(frames, mid, sub), frames)
        if measured[mid][key] >= target:
            high = mid
        else:
            low = mid + 1
    return (low, measured[low], True) if low <= 100 else (100, measured[100], False)


def palette_quality(frames, indices, palette):
    """``quality.compare`` of what a GIF shows, ``palette[indices]``, against the frames it was made from — what ``colors``, ``dither`` and ``palette`` of
    ``palettize`` cost.  ``indices`` uint8 [F, H, W], ``palette`` uint8 [K, 3] or [F, K, 3], on the frames' device; one gather there, two launches, ONE host read."""
    f, h, w = _check_frames(frames)
    if not torch.is_tensor(indices) or indices.dtype != torch.uint8 or tuple(indices.shape) != (f, h, w) or indices.device != frames.device:
        raise ValueError(f'palette_quality: indices must be uint8 [{f}, {h}, {w}] on {frames.device}')
    if not torch.is_tensor(palette) or palette.dtype != torch.uint8 or palette.ndim not in (2, 3) or palette.shape[-1] != 3 or palette.device != frames.device \
            or (palette.ndim == 3 and palette.shape[0] != f):
        raise ValueError(f'palette_quality: palette must be uint8 [K, 3] or [{f}, K, 3] on {frames.device}')
    from . import quality as Q
    idx = indices.long().clamp(max=palette.shape[-2] - 1)                        # (an index past the palette shows its last row: no read out of bounds)
    shown = palette[idx] if palette.ndim == 2 else torch.gather(palette, 1, idx.reshape(f, -1, 1).expand(-1, -1, 3)).reshape(f, h, w, 3)
    return Q.compare(shown, frames)


# ---- the way back from a file: entropy decoding ----------------------------------------------------------------------------------------------------
# ``jpeg_decode`` starts from coefficients; a file holds their Huffman codes.  The parser is host work over a few hundred header bytes; the decoding of
# the scan is ``p3d_video_jpeg_unscan``, a lane per restart interval, and an integer function of the bytes: p3d_video.h states it, the numpy formulation
# here is the definition, the device result equals it.
JPEG_LOOKUP_BITS, JPEG_TABLE_WORDS = HEADER.constants['P3D_VIDEO_JPEG_LOOKUP_BITS'], HEADER.constants['P3D_VIDEO_JPEG_TABLE_WORDS']
JPEG_STATUS = {name: HEADER.constants['P3D_VIDEO_JPEG_STATUS_' + name] for name in ('NO_CODE', 'RUN', 'SIZE', 'EXHAUSTED', 'LEFTOVER')}
JpegInfo = collections.namedtuple('JpegInfo', 'h w subsampling components tables huffman restart scan intervals')
JpegInfo.__doc__ = """What ``jpeg_parse`` reads from a baseline JPEG: ``h``, ``w``; ``subsampling`` '4:4:4' or '4:2:0' and ``components`` 3 — or 1, a grey stream,
laid out as 4:4:4 whose chroma tables equal its luma tables; ``tables`` (luma, chroma) uint8 [64] in zigzag order, as ``jpeg_tables`` returns them;
``huffman`` the (BITS, HUFFVAL) of DC luma, DC chroma, AC luma, AC chroma; ``restart`` MCUs an interval, 0: none; ``scan`` (begin, end) of the entropy-coded
bytes in the stream; ``intervals`` int64 numpy [n, 2]: (begin, end) of every restart interval, markers left out."""
_SOF_NAMES = {0xC1: 'extended sequential (SOF1)', 0xC2: 'progressive (SOF2)', 0xC3: 'lossless (SOF3)', 0xC5: 'differential sequential (SOF5)',
              0xC6: 'differential progressive (SOF6)', 0xC7: 'differential lossless (SOF7)', 0xC9: 'arithmetic coding (SOF9)', 0xCA: 'arithmetic coding (SOF10)',
              0xCB: 'arithmetic coding (SOF11)', 0xCD: 'arithmetic coding (SOF13)', 0xCE: 'arithmetic coding (SOF14)', 0xCF: 'arithmetic coding (SOF15)',
              0xCC: 'arithmetic coding (DAC)'}


def _check_dht(bits, values, what='jpeg_decode_tables'):
    bits, values = tuple(int(b) for b in bits), tuple(int(v) for v in values)
    if len(bits) != 16 or min(bits) < 0 or sum(bits) != len(values) or any(not 0 <= v <= 255 for v in values):
        raise ValueError(f'{what}: a Huffman table is 16 counts and as many symbols 0 .. 255 as they add up to')
    if len(values) > 256:
        raise ValueError(f'{what}: a Huffman table lists {len(values)} symbols, more than 256')
    if sum(n << (16 - length) for length, n in enumerate(bits, start=1)) > 1 << 16:
        raise ValueError(f'{what}: the counts {bits} over-subscribe the code space')
    return bits, values


_decode_tables = {}


def jpeg_decode_tables(bits, values):
    """int32 [JPEG_TABLE_WORDS] on the host (the bits of uint32 words): what ``p3d_video_jpeg_unscan`` reads for ONE Huffman table given as a DHT segment
    states it — ``bits``, the number of codes of every length 1 .. 16, and ``values``, the symbols in code order.  The format is p3d_video.h's: a lookup by
    8-bit prefix (length << 16 | symbol, 0: no code that short), then per length the last code + 1 and the index of its first symbol minus its first code
    (Annex F's maxcode and valptr - mincode), then the symbols.  ValueError for counts that over-subscribe the code space or list more than 256 symbols."""
    key = _check_dht(bits, values)
    if key not in _decode_tables:
        bits, values = key
        words = np.zeros(JPEG_TABLE_WORDS, dtype=np.int64)
        lookup = 1 << JPEG_LOOKUP_BITS
        code, k = 0, 0
        for length, n in enumerate(bits, start=1):                                # the canonical assignment of Annex C
            if n:
                words[lookup + length - 1], words[lookup + 16 + length - 1] = code + n, (k - code) & 0xFFFFFFFF
            for i in range(n if length <= JPEG_LOOKUP_BITS else 0):
                shift = JPEG_LOOKUP_BITS - length
                words[(code + i) << shift:(code + i + 1) << shift] = length << 16 | values[k + i]
            code, k = (code + n) << 1, k + n
        for i, v in enumerate(values):
            words[lookup + 32 + (i >> 2)] |= v << (8 * (i & 3))
        _decode_tables[key] = torch.from_numpy(words.astype(np.uint32).view(np.int32))
    return _decode_tables[key]


def jpeg_parse(stream):
    """The ``JpegInfo`` of one JPEG given as ``bytes``: everything ``jpeg_unscan`` and ``jpeg_decode`` need, read from the segments before the scan, and the
    byte range of every restart interval, found by one vectorised search of the scan for 0xFF followed by anything but 0x00 (which is data).  ValueError,
    naming the reason, for what the decoder does not serve — anything but baseline sequential 8-bit Huffman coding (SOF1, progressive, arithmetic), 16-bit
    quantisation tables, 4 components, sampling other than all 1 x 1 or Y 2 x 2 with chroma 1 x 1, more than one scan or a scan that does not interleave
    all components, DNL — and for a stream that is not whole: a header that ends early, a DHT that over-subscribes the code space or lists more than 256
    symbols, RSTm out of the cyclic order 0 .. 7, an interval count other than ceil(n_mcu / interval), any other marker inside the scan, no EOI."""
    if not isinstance(stream, (bytes, bytearray, memoryview)):
        raise ValueError(f'jpeg_parse: stream must be bytes, got {type(stream).__name__}')
    stream = bytes(stream)
    if stream[:2] != b'\xff\xd8':
        raise ValueError('jpeg_parse: not a JPEG: the stream does not begin with SOI')
    at, dqt, dht, frame, restart, scan = 2, {}, {}, None, 0, None
    while scan is None:
        while at + 1 < len(stream) and stream[at] == 0xFF and stream[at + 1] == 0xFF:      # fill bytes before a marker
            at += 1
        if at + 4 > len(stream):
            raise ValueError(f'jpeg_parse: the stream ends inside its header, at byte {at}')
        if stream[at] != 0xFF:
            raise ValueError(f'jpeg_parse: no marker at byte {at} of the header')
        marker, size = stream[at + 1], int.from_bytes(stream[at + 2:at + 4], 'big')
        if marker in _SOF_NAMES:
            raise ValueError(f'jpeg_parse: {_SOF_NAMES[marker]} is not baseline sequential Huffman coding')
        if marker == 0xDC:
            raise ValueError('jpeg_parse: DNL (the height comes after the scan) is not served')
        if marker == 0xD9 or marker == 0xD8 or 0xD0 <= marker <= 0xD7 or marker == 0x01 or marker == 0x00:
            raise ValueError(f'jpeg_parse: the marker 0x{marker:02X} at byte {at} has no place in a header')
        if size < 2 or at + 2 + size > len(stream):
            raise ValueError(f'jpeg_parse: the stream ends inside its header: the segment 0x{marker:02X} at byte {at} runs past the end')
        p = stream[at + 4:at + 2 + size]
        at += 2 + size
        if marker == 0xDB:
            while p:
                if p[0] >> 4:
                    raise ValueError('jpeg_parse: a 16-bit quantisation table (DQT) is not baseline 8-bit')
                if len(p) < 65:
                    raise ValueError('jpeg_parse: a DQT segment ends inside a table')
                dqt[p[0] & 15], p = p[1:65], p[65:]
        elif marker == 0xC4:
            while p:
                if len(p) < 17 or len(p) < 17 + sum(p[1:17]):
                    raise ValueError('jpeg_parse: a DHT segment ends inside a table')
                n = sum(p[1:17])
                dht[p[0]], p = _check_dht(p[1:17], p[17:17 + n], 'jpeg_parse: DHT'), p[17 + n:]
        elif marker == 0xC0:
            if frame is not None:
                raise ValueError('jpeg_parse: a second SOF0')
            if len(p) < 6 or len(p) != 6 + 3 * p[5]:
                raise ValueError('jpeg_parse: SOF0 has the wrong length')
            if p[0] != 8:
                raise ValueError(f'jpeg_parse: {p[0]}-bit samples are not baseline 8-bit')
            if p[5] == 4:
                raise ValueError('jpeg_parse: 4 components (CMYK / YCCK) are not served')
            if p[5] not in (1, 3):
                raise ValueError(f'jpeg_parse: {p[5]} components: 1 (grey) or 3 (Y Cb Cr) are served')
            frame = (int.from_bytes(p[1:3], 'big'), int.from_bytes(p[3:5], 'big'), [tuple(p[6 + 3 * i:9 + 3 * i]) for i in range(p[5])])
            if frame[0] == 0:
                raise ValueError('jpeg_parse: a height of 0 leaves it to DNL, which is not served')
            if frame[1] == 0:
                raise ValueError('jpeg_parse: a width of 0')
        elif marker == 0xDD:
            if len(p) != 2:
                raise ValueError('jpeg_parse: DRI has the wrong length')
            restart = int.from_bytes(p, 'big')
        elif marker == 0xDA:
            if frame is None:
                raise ValueError('jpeg_parse: SOS before SOF0')
            scan = p
    h, w, components = frame
    nc = len(components)
    if not scan or len(scan) != 4 + 2 * scan[0]:
        raise ValueError('jpeg_parse: SOS has the wrong length')
    if scan[0] != nc or [scan[1 + 2 * i] for i in range(nc)] != [c[0] for c in components]:
        raise ValueError(f'jpeg_parse: the scan holds {scan[0]} of {nc} components: more than one scan, or a scan that is not interleaved, is not served')
    if tuple(scan[1 + 2 * nc:]) != (0, 63, 0):
        raise ValueError('jpeg_parse: the scan is not the whole band 0 .. 63 at full precision: not baseline sequential')
    sampling = [c[1] for c in components]
    if nc == 1 or sampling == [0x11, 0x11, 0x11]:                                     # (one component: its sampling factors play no part, T.81 A.2.2)
        subsampling = '4:4:4'
    elif sampling == [0x22, 0x11, 0x11]:
        subsampling = '4:2:0'
    else:
        raise ValueError(f'jpeg_parse: sampling factors {" ".join(f"{s >> 4}x{s & 15}" for s in sampling)}: all 1x1 (4:4:4) or Y 2x2 with chroma 1x1 (4:2:0) are served')
    selected = []
    for i, c in enumerate(components):
        tdta = scan[2 + 2 * i]
        if c[2] not in dqt or (tdta >> 4) not in dht or (0x10 | (tdta & 15)) not in dht:
            raise ValueError(f'jpeg_parse: component {c[0]} selects a table the stream does not define')
        selected.append((bytes(dqt[c[2]]), dht[tdta >> 4], dht[0x10 | (tdta & 15)]))
    if nc == 3 and selected[1] != selected[2]:
        raise ValueError('jpeg_parse: Cb and Cr select different tables: one chroma set is served')
    luma, chroma = selected[0], selected[-1]
    tables = tuple(torch.tensor(list(t[0]), dtype=torch.uint8) for t in (luma, chroma))
    huffman = (luma[1], chroma[1], luma[2], chroma[2])

    body = np.frombuffer(stream, dtype=np.uint8, offset=at)
    markers = np.flatnonzero((body[:-1] == 0xFF) & (body[1:] != 0)) if body.shape[0] > 1 else np.zeros([0], dtype=np.int64)
    kinds = body[markers + 1]
    others = np.flatnonzero((kinds < 0xD0) | (kinds > 0xD7))
    if others.shape[0] == 0:
        raise ValueError('jpeg_parse: the scan has no EOI')
    last = int(others[0])
    if kinds[last] != 0xD9:
        reason = {0xDA: 'a second scan (SOS)', 0xDC: 'DNL', 0xC4: 'tables (DHT) for a second scan', 0xFF: 'a fill byte (0xFF 0xFF)'}.get(int(kinds[last]), 'a marker')
        raise ValueError(f'jpeg_parse: {reason}, 0xFF 0x{int(kinds[last]):02X}, inside the scan at byte {at + int(markers[last])}: only RSTm and EOI are served')
    rst, end = markers[:last], int(markers[last])
    if not np.array_equal(kinds[:last] - 0xD0, np.arange(last) & 7):
        raise ValueError(f'jpeg_parse: the restart markers are out of the cyclic order 0 .. 7: {[int(k) - 0xD0 for k in kinds[:last]][:16]}')
    _, n_mcu, _, _ = jpeg_layout(h, w, subsampling)
    expected = -(-n_mcu // restart) if restart else 1
    if last + 1 != expected:
        raise ValueError(f'jpeg_parse: {last + 1} restart intervals, but {n_mcu} MCUs at an interval of {restart} make {expected}')
    intervals = at + np.stack([np.concatenate([[0], rst + 2]), np.concatenate([rst, [end]])], axis=1).astype(np.int64)
    return JpegInfo(h, w, subsampling, nc, tables, huffman, restart, (at, at + end), intervals)


def _jpeg_unscan_numpy(data, ranges, tables, table_of_frame, n_mcu, bpm, coded, restart):
    """The rules of p3d_video.h with every interval a row of numpy arrays: one step decodes ONE coefficient (a symbol and its extra bits) of every interval
    still running.  ``data`` uint8 [n], ``ranges`` int64 [F, n_intervals, 2], ``tables`` [n_sets, 4, JPEG_TABLE_WORDS] as uint32 values in int64."""
    f, n_intervals = ranges.shape[:2]
    lanes = f * n_intervals
    begin = np.clip(ranges[..., 0].reshape(-1), 0, data.shape[0])
    end = np.clip(ranges[..., 1].reshape(-1), begin, data.shape[0])
    # the data bytes of every interval — a 0x00 straight after a 0xFF of the interval dropped — each interval followed by 8 zero bytes: the bits past its end
    n_raw = end - begin
    start = np.cumsum(n_raw) - n_raw
    lane_of = np.repeat(np.arange(lanes), n_raw)
    raw = data[np.arange(int(n_raw.sum())) - start[lane_of] + begin[lane_of]].astype(np.int64)
    first = np.zeros(raw.shape[0], dtype=bool)
    first[start[n_raw > 0]] = True
    keep = ~((raw == 0) & np.concatenate([[False], raw[:-1] == 0xFF]) & ~first)
    lane_of = lane_of[keep]
    n_bytes = np.bincount(lane_of, minlength=lanes)
    base = np.cumsum(n_bytes + 8) - (n_bytes + 8)
    padded = np.zeros(int((n_bytes + 8).sum()), dtype=np.int64)
    padded[base[lane_of] + np.arange(lane_of.shape[0]) - (np.cumsum(n_bytes) - n_bytes)[lane_of]] = raw[keep]
    total = 8 * n_bytes

    frame, interval = np.arange(lanes) // n_intervals, np.arange(lanes) % n_intervals
    mcu0 = interval * restart
    n_blocks = np.minimum(restart, n_mcu - mcu0) * coded
    table_base = np.clip(table_of_frame[frame], 0, tables.shape[0] - 1) * 4 * JPEG_TABLE_WORDS
    words = tables.reshape(-1)
    lookup, longer = 1 << JPEG_LOOKUP_BITS, np.arange(JPEG_LOOKUP_BITS + 1, 17)
    bit, block, z = np.zeros(lanes, dtype=np.int64), np.zeros(lanes, dtype=np.int64), np.zeros(lanes, dtype=np.int64)
    pred, status = np.zeros([lanes, 3], dtype=np.int64), np.zeros(lanes, dtype=np.int64)
    out = np.zeros(f * n_mcu * bpm * 64, dtype=np.int16)

    def peek(a, at):                                                              # the 16 bits from bit ``at`` of the lanes ``a``
        i = base[a] + (at >> 3)
        return ((padded[i] << 16 | padded[i + 1] << 8 | padded[i + 2]) >> (8 - (at & 7))) & 0xFFFF
    a = np.flatnonzero(n_blocks > 0)
    while a.shape[0]:
        k = block[a] % coded
        comp = k if bpm == 3 else np.maximum(k - 3, 0)
        dc = z[a] == 0
        t = table_base[a] + (np.where(dc, 0, 2) + (comp > 0)) * JPEG_TABLE_WORDS
        bits = peek(a, bit[a])
        entry = words[t + (bits >> (16 - JPEG_LOOKUP_BITS))]
        length, symbol = entry >> 16, entry & 255
        no_code = np.zeros(a.shape[0], dtype=bool)
        slow = np.flatnonzero((length < 1) | (length > JPEG_LOOKUP_BITS))
        if slow.shape[0]:                                                         # Annex F: the first length whose prefix is below the limit
            codes = bits[slow, None] >> (16 - longer)
            hit = codes < words[t[slow, None] + lookup + longer - 1]
            l = hit.argmax(axis=1)
            offset = words[t[slow] + lookup + 16 + longer[l] - 1]
            at = codes[np.arange(slow.shape[0]), l] + np.where(offset >= 1 << 31, offset - (1 << 32), offset)
            found = hit.any(axis=1) & (at >= 0) & (at < 256)
            at = np.clip(at, 0, 255)
            length[slow] = np.where(found, longer[l], 16)
            symbol[slow] = (words[t[slow] + lookup + 32 + (at >> 2)] >> (8 * (at & 3))) & 255
            no_code[slow] = ~found
        flags = np.where(no_code, JPEG_STATUS['NO_CODE'], 0)
        bit_after = bit[a] + length
        flags |= np.where(bit_after > total[a], JPEG_STATUS['EXHAUSTED'], 0)
        size, run = np.where(dc, symbol, symbol & 15), np.where(dc, 0, symbol >> 4)
        eob, zrl = ~dc & (size == 0) & (run == 0), ~dc & (size == 0) & (run == 15)
        bad = np.where(dc, size > 11, (size > 10) | ((size == 0) & ~eob & ~zrl))
        flags = np.where((flags == 0) & bad, JPEG_STATUS['SIZE'], flags)
        size = np.where(flags == 0, size, 0)
        extra = peek(a, bit_after) >> (16 - size)
        bit_after = bit_after + size
        flags = np.where((flags == 0) & (bit_after > total[a]), JPEG_STATUS['EXHAUSTED'], flags)
        value = np.where(size == 0, 0, np.where(extra >= (1 << np.maximum(size - 1, 0)), extra, extra - (1 << size) + 1))
        position = np.where(dc | eob, z[a], z[a] + np.where(zrl, 16, run))
        flags = np.where((flags == 0) & (position > 63), JPEG_STATUS['RUN'], flags)
        good = flags == 0
        status[a] |= flags
        value = np.where(dc, np.clip(pred[a, comp] + value, -32768, 32767), value)
        store = good & ~eob & ~zrl
        lane = a[store]
        pred[lane[dc[store]], comp[store][dc[store]]] = value[store][dc[store]]
        out[(((frame[lane] * n_mcu + mcu0[lane] + block[lane] // coded) * bpm + k[store]) * 64 + position[store])] = value[store]
        position = np.where(eob, 64, np.where(zrl, position, position + 1))
        done = position > 63                                                      # the block is complete
        bit[a], z[a] = bit_after, np.where(done, 0, position)
        block[a] += done
        finished = good & done & (block[a] == n_blocks[a])
        status[a[finished]] |= np.where((total[a[finished]] - bit[a[finished]]) >> 3 > 1, JPEG_STATUS['LEFTOVER'], 0)
        a = a[good & ~finished]
    return out.reshape(f, n_mcu, bpm, 64), status.reshape(f, n_intervals).astype(np.int32)


def _annex_k_decode_tables():
    return (torch.stack([jpeg_decode_tables(*t) for t in _ANNEX_K])[None],)


def jpeg_unscan(data, ranges, h, w, subsampling='4:2:0', tables=None, table_of_frame=None, restart=JPEG_RESTART, components=3):
    """``(coefficients int16 [F, n_mcu, 3 or 6, 64], status int32 [F, n_intervals])``: the inverse of ``jpeg_scan`` — and of any baseline coder that cuts its
    scans into restart intervals.  ``data`` uint8 [n]: the bytes of all scans; ``ranges`` int64 [F, n_intervals, 2]: the (begin, end) of every interval of
    every frame in ``data``, markers left out (``jpeg_parse``'s ``intervals``, shifted to where the scan went), with n_intervals = ceil(n_mcu / restart);
    ``restart`` 0 means none: one interval of the whole frame.  ``tables`` int32 [n_sets, 4, JPEG_TABLE_WORDS]: sets of ``jpeg_decode_tables`` in the order DC
    luma, DC chroma, AC luma, AC chroma — optimised tables differ from file to file — and ``table_of_frame`` int32 [F] the set of every frame; by default the
    Annex K tables of ``jpeg_scan`` for all.  ``components`` 1: grey streams, laid out as 4:4:4 with zero chroma blocks.  The coefficients are in
    ``jpeg_coefficients``' layout, so ``jpeg_decode`` takes them as they are.  ``status`` is 0 for an interval that decoded cleanly, else the ``JPEG_STATUS``
    bits that stopped it — what it had decoded stays, the rest of it is zero, and no other interval is touched.  Device tensors: one asynchronous fill and
    ONE launch of ``p3d_video_jpeg_unscan``, a lane per interval, and no synchronisation; CPU tensors: the numpy formulation.  The parallel unit is the
    interval: a stream without restart markers is one lane a frame — correct, but slow (DESIGN.md section 2.1y has the figures)."""
    sub = _check_subsampling(subsampling)
    h, w = int(h), int(w)
    _, n_mcu, bpm, _ = jpeg_layout(h, w, sub)
    if components not in (1, 3) or (components == 1 and sub):
        raise ValueError(f'jpeg_unscan: components is 3, or 1 at 4:4:4, got {components!r} at subsampling {subsampling!r}')
    if isinstance(restart, bool) or int(restart) != restart or int(restart) < 0:
        raise ValueError(f'jpeg_unscan: restart must be an integer >= 0, got {restart!r}')
    restart = min(int(restart), n_mcu) or n_mcu
    n_intervals = -(-n_mcu // restart) if n_mcu else 0
    if not torch.is_tensor(data) or data.dtype != torch.uint8 or data.ndim != 1:
        raise ValueError('jpeg_unscan: data must be a uint8 [n] tensor')
    device = data.device
    if not torch.is_tensor(ranges) or ranges.dtype != torch.int64 or ranges.ndim != 3 or ranges.shape[2] != 2:
        raise ValueError('jpeg_unscan: ranges must be an int64 [F, n_intervals, 2] tensor')
    f = ranges.shape[0]
    if h < 0 or w < 0 or f * h * w >= MAX_PIXELS:
        raise ValueError(f'jpeg_unscan: {f} x {h} x {w} pixels are negative or reach 2^31')
    if f * h * w == 0:
        return torch.zeros([f, 0, bpm, 64], dtype=torch.int16, device=device), torch.zeros([f, 0], dtype=torch.int32, device=device)
    if ranges.shape[1] != n_intervals:
        raise ValueError(f'jpeg_unscan: {n_mcu} MCUs at an interval of {restart} are {n_intervals} intervals a frame, got ranges for {ranges.shape[1]}')
    if tables is None:
        tables, = _device_tables('decode tables', device, _annex_k_decode_tables)
    if not torch.is_tensor(tables) or tables.dtype != torch.int32 or tables.ndim != 3 or tuple(tables.shape[1:]) != (4, JPEG_TABLE_WORDS) or tables.shape[0] < 1:
        raise ValueError(f'jpeg_unscan: tables must be an int32 [n_sets, 4, {JPEG_TABLE_WORDS}] tensor')
    if table_of_frame is None:
        table_of_frame = torch.zeros([f], dtype=torch.int32, device=device)
    if not torch.is_tensor(table_of_frame) or table_of_frame.dtype != torch.int32 or tuple(table_of_frame.shape) != (f,):
        raise ValueError(f'jpeg_unscan: table_of_frame must be an int32 [{f}] tensor')
    if not data.is_cuda:
        out, status = _jpeg_unscan_numpy(data.contiguous().numpy(), ranges.cpu().numpy(), tables.cpu().contiguous().numpy().view(np.uint32).astype(np.int64),
                                         table_of_frame.cpu().numpy().astype(np.int64), n_mcu, bpm, 1 if components == 1 else bpm, restart)
        return torch.from_numpy(out), torch.from_numpy(status)
    data, ranges, tables, table_of_frame = (t.to(device).contiguous() for t in (data, ranges, tables, table_of_frame))
    out = torch.empty([f, n_mcu, bpm, 64], dtype=torch.int16, device=device)
    status = torch.empty([f, n_intervals], dtype=torch.int32, device=device)
    with _lib.kernel_timer('video_jpeg_unscan', out):
        code = video_lib().p3d_video_jpeg_unscan(_lib.ptr(data), data.shape[0], _lib.ptr(ranges), _lib.ptr(tables), tables.shape[0], _lib.ptr(table_of_frame),
                                                 f, h, w, sub, int(components), restart, _lib.ptr(out), _lib.ptr(status), _lib.stream_of(out))
    _check(code, 'video_jpeg_unscan')
    return out, status


def _upload(array, device):
    """A host array on ``device`` without a wait: through pinned memory, which the copy may leave behind it."""
    t = torch.from_numpy(np.ascontiguousarray(array))
    return t.pin_memory().to(device, non_blocking=True) if torch.device(device).type == 'cuda' else t


def jpeg_status_names(bits):
    """The names of the ``JPEG_STATUS`` bits set in ``bits``."""
    return [name for name, bit in JPEG_STATUS.items() if int(bits) & bit]


def decode_jpeg(streams, device=None, errors='raise'):
    """uint8 [F, H, W, 3] on ``device`` (default: the host): the pictures of a list of baseline JPEG ``bytes`` of ONE size — ours (``encode_jpeg``, the frames
    of ``read_avi``) or anybody's that ``jpeg_parse`` accepts; grey streams show r = g = b.  The headers are parsed on the host, the scans go to the device
    in ONE copy, the frames are grouped by geometry (subsampling, restart interval) for ``jpeg_unscan`` — a fill and a launch a group — and every run of
    frames with equal quantisation tables is one ``jpeg_decode`` (two launches) into its rows of the result.  What ``jpeg_decode`` shows for our own streams
    is ``jpeg_reconstruct`` of the frames they were made from, byte for byte; against libjpeg's decoder a level here and there differs.
    ``errors='raise'``: a scan that does not decode cleanly is a ValueError naming frame, interval and reason — one small device -> host copy.
    ``errors='status'``: ``(frames, status)`` with status int32 [F, the most intervals of a frame] (``JPEG_STATUS`` bits, 0: clean or no such interval) on the
    device, and no synchronisation; a damaged interval shows what it decoded and zeros (grey) after it."""
    if errors not in ('raise', 'status'):
        raise ValueError(f"decode_jpeg: errors is 'raise' or 'status', got {errors!r}")
    device = torch.device('cpu' if device is None else device)
    infos = [jpeg_parse(s) for s in streams]
    if not infos:
        raise ValueError('decode_jpeg: no stream')
    h, w = infos[0].h, infos[0].w
    for i, info in enumerate(infos):
        if (info.h, info.w) != (h, w):
            raise ValueError(f'decode_jpeg: stream {i} is {info.h} x {info.w}, stream 0 {h} x {w}: one call, one size')
    f = len(infos)
    if f * h * w >= MAX_PIXELS:
        raise ValueError(f'decode_jpeg: {f} x {h} x {w} pixels reach 2^31')
    sizes = np.array([0] + [info.scan[1] - info.scan[0] for info in infos], dtype=np.int64)
    offsets = np.cumsum(sizes)
    data = _upload(np.frombuffer(bytearray().join(s[info.scan[0]:info.scan[1]] for s, info in zip(streams, infos)), dtype=np.uint8), device)
    sets, quant = {}, {}                                                          # the distinct Huffman sets and quantisation pairs, in order of appearance
    set_of = [sets.setdefault(info.huffman, len(sets)) for info in infos]
    quant_of = [quant.setdefault(tuple(bytes(t.tolist()) for t in info.tables), len(quant)) for info in infos]
    tables = _upload(torch.stack([torch.stack([jpeg_decode_tables(*t) for t in key]) for key in sets]).numpy(), device)
    quant_tables = _upload(np.array([[list(t) for t in key] for key in quant], dtype=np.uint8), device)
    frames = torch.empty([f, h, w, 3], dtype=torch.uint8, device=device)
    status = torch.zeros([f, max(info.intervals.shape[0] for info in infos)], dtype=torch.int32, device=device)
    groups = {}
    for i, info in enumerate(infos):
        groups.setdefault((info.subsampling, info.components, info.restart), []).append(i)
    for (subsampling, components, restart), members in groups.items():
        ranges = _upload(np.stack([infos[i].intervals - infos[i].scan[0] + offsets[i] for i in members]), device)
        table_of_frame = _upload(np.array([set_of[i] for i in members], dtype=np.int32), device)
        coefficients, group_status = jpeg_unscan(data, ranges, h, w, subsampling, tables, table_of_frame, restart, components)
        whole = members == list(range(f))                                         # the usual case: one group
        if whole:
            status[:, :group_status.shape[1]] = group_status
        else:
            status[_upload(np.array(members), device), :group_status.shape[1]] = group_status
        a = 0
        while a < len(members):                                                   # runs of frames that are neighbours in the result and share their tables
            b = a + 1
            while b < len(members) and members[b] == members[b - 1] + 1 and quant_of[members[b]] == quant_of[members[a]]:
                b += 1
            jpeg_decode(coefficients[a:b], quant_tables[quant_of[members[a]]], h, w, subsampling, out=frames[members[a]:members[a] + b - a])
            a = b
    if errors == 'status':
        return frames, status
    bad = status.cpu().nonzero()
    if bad.shape[0]:
        i, j = bad[0].tolist()
        raise ValueError(f'decode_jpeg: frame {i}, restart interval {j} does not decode: {", ".join(jpeg_status_names(status[i, j]))}'
                         f' ({bad.shape[0]} damaged interval{"s" if bad.shape[0] > 1 else ""} in all)')
    return frames


def load_jpeg(path, device=None):
    """uint8 [H, W, 3] on ``device``: the picture of a baseline JPEG file (``decode_jpeg``)."""
    with open(path, 'rb') as fh:
        return decode_jpeg([fh.read()], device)[0]


def decode_avi(path, device=None):
    """``(frames uint8 [F, H, W, 3] on device, fps)`` of a Motion-JPEG AVI: ``decode_jpeg`` of ``read_avi``'s streams — the clip ``save_avi`` wrote, as its
    viewers see it, without a host decoder in the loop."""
    streams, fps, (w, h) = read_avi(path)
    frames = decode_jpeg(streams, device)
    if tuple(frames.shape[1:3]) != (h, w):
        raise ValueError(f'decode_avi: the stream header says {h} x {w}, the frames are {frames.shape[1]} x {frames.shape[2]}')
    return frames, fps


def check_avi(path, frames, quality=90, subsampling='4:2:0'):
    """The dict of ``quality.compare(decode_avi(path)[0], frames)`` plus ``'exact'``: whether the file shows ``jpeg_reconstruct(frames, quality, subsampling)``
    byte for byte — that the clip on disk is the clip the setting promised.  On the frames' device."""
    from . import quality as Q
    frames = torch.as_tensor(frames)
    shown = decode_avi(path, frames.device)[0]
    if shown.shape != frames.shape:
        raise ValueError(f'check_avi: the file holds {tuple(shown.shape)}, the frames are {tuple(frames.shape)}')
    metrics = Q.compare(shown, frames)
    metrics['exact'] = bool(torch.equal(shown, jpeg_reconstruct(frames, quality, subsampling)))
    return metrics


# ---- lossless frames: PNG and APNG -----------------------------------------------------------------------------------------------------------
# Every frame a zlib stream made where the frames are, in three stages that p3d_video.h states in integers: the row filter, the symbol counts of every
# segment, the bytes.  Between count and emit the host makes one Huffman code a frame; what does not touch pixels (chunks, CRC-32) is host work too.
PNG_SYMBOLS, PNG_STATS, PNG_HEADER_WORDS, PNG_ADAPTIVE = (HEADER.constants['P3D_VIDEO_PNG_' + k] for k in ('SYMBOLS', 'STATS', 'HEADER_WORDS', 'ADAPTIVE'))
PNG_SEGMENT_BYTES = 32768                            # filtered bytes of a segment, about: the unit of parallel work (DESIGN.md section 2.1v records the choice)
PNG_MODES = {'L': (1, 0, 8), 'LA': (2, 4, 8), 'RGB': (3, 2, 8), 'RGBA': (4, 6, 8), 'P': (1, 3, 8), 'I;16': (2, 0, 16)}      # mode: bytes a pixel, colour type, depth
PNG_FILTERS = {'none': 0, 'sub': 1, 'up': 2, 'average': 3, 'paeth': 4, 'adaptive': PNG_ADAPTIVE}
PNG_MAX_MATCH = 258
_PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'
_ADLER = 65521
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)       # RFC 1951 section 3.2.7: the order of the code-length code's lengths
_LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)      # of the symbols 257 .. 285
_LENGTH_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)


def _length_tables():
    """(symbol, extra bits, extra value) of every match length 0 .. 258, from the RFC's table (entries below 3 are unused)."""
    symbol, bits, value = (np.zeros(PNG_MAX_MATCH + 1, dtype=np.int64) for _ in range(3))
    for length in range(3, PNG_MAX_MATCH + 1):
        i = max(j for j, base in enumerate(_LENGTH_BASE) if base <= length)
        symbol[length], bits[length], value[length] = 257 + i, _LENGTH_EXTRA[i], length - _LENGTH_BASE[i]
    return symbol, bits, value


_LEN_SYMBOL, _LEN_BITS, _LEN_VALUE = _length_tables()


def _check_filter(filter):
    if isinstance(filter, str) and filter in PNG_FILTERS:
        return PNG_FILTERS[filter]
    if isinstance(filter, bool) or isinstance(filter, str) or int(filter) != filter or not 0 <= int(filter) <= PNG_ADAPTIVE:
        raise ValueError(f"filter must be 0 .. {PNG_ADAPTIVE} or one of {', '.join(PNG_FILTERS)}, got {filter!r}")
    return int(filter)


def _bpp(frames):
    return frames.shape[3] if frames.ndim == 4 else 1


def _check_filtered(filtered, what):
    if not torch.is_tensor(filtered) or filtered.dtype != torch.uint8 or filtered.ndim != 3:
        raise ValueError(f'{what}: filtered must be a uint8 [F, H, 1 + W bpp] tensor (png_filter)')
    f, h, r = filtered.shape
    if f * h * r >= MAX_PIXELS:
        raise ValueError(f'{what}: {f} x {h} x {r} filtered bytes reach 2^31')
    return f, h, r


def _check_segment_rows(segment_rows):
    if isinstance(segment_rows, bool) or int(segment_rows) != segment_rows or int(segment_rows) < 1:
        raise ValueError(f'segment_rows must be an integer >= 1, got {segment_rows!r}')
    return int(segment_rows)


def png_segment_rows(w, bpp):
    """The rows of a segment for pictures ``w`` pixels of ``bpp`` bytes wide: max(1, PNG_SEGMENT_BYTES // (1 + w bpp))."""
    return max(1, PNG_SEGMENT_BYTES // (1 + int(w) * int(bpp)))


def _png_filter_numpy(x, bpp, filt):
    """uint8 [H, 1 + n] of ONE frame ``x`` int64 [H, n]: the header's filter rule, every candidate in full."""
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, bpp:], b[1:], c[1:, bpp:] = x[:, :-bpp], x[:-1], x[:-1, :-bpp]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    residuals = np.stack([(x - pred) & 255 for pred in (0, a, b, (a + b) >> 1, paeth)])
    if filt == PNG_ADAPTIVE:
        types = np.where(residuals < 128, residuals, 256 - residuals).sum(axis=2).argmin(axis=0)      # argmin: the first, so the lowest type on a tie
    else:
        types = np.full(x.shape[0], filt, dtype=np.int64)
    chosen = np.take_along_axis(residuals, types[None, :, None], axis=0)[0]
    return np.concatenate([types[:, None], chosen], axis=1).astype(np.uint8)


def png_filter(frames, filter='adaptive'):
    """uint8 [F, H, 1 + W bpp]: every row as its filter type and its residuals — the PNG specification's None, Sub, Up, Average and Paeth, the row above a
    frame's first being zeros.  Frames uint8 [F, H, W] (bpp 1) or [F, H, W, bpp] (bpp 2 .. 4) with contiguous pixels and any pitches; ``filter`` 0 .. 4 or
    its name forces a type, 'adaptive' (5) takes per row the type with the smallest sum of |residual as int8|, the lowest on a tie (libpng's heuristic).
    Device tensors: ONE ``p3d_video_png_filter`` launch; CPU tensors: the numpy formulation."""
    f, h, w = _check_frames(frames, 'png_filter', (1, 2, 3, 4))
    bpp, filt = _bpp(frames), _check_filter(filter)
    if f * h * (1 + w * bpp) >= MAX_PIXELS:
        raise ValueError(f'png_filter: {f} x {h} rows of {1 + w * bpp} filtered bytes reach 2^31')
    if f * h * w == 0:
        return torch.zeros([f, h, 1 + w * bpp], dtype=torch.uint8, device=frames.device)
    if not frames.is_cuda:
        return torch.from_numpy(np.stack([_png_filter_numpy(x.reshape(h, w * bpp).to(torch.int64).numpy(), bpp, filt) for x in frames]))
    out = torch.empty([f, h, 1 + w * bpp], dtype=torch.uint8, device=frames.device)
    with _lib.kernel_timer('video_png_filter', out):
        code = video_lib().p3d_video_png_filter(*_clip(frames), bpp, filt, _lib.ptr(out), _lib.stream_of(out))
    _check(code, 'video_png_filter')
    return out


def _png_tokens(b, segment_bytes):
    """(literals, match) per byte of ONE frame's filtered bytes ``b`` int64 [n], cut into segments of ``segment_bytes``: how many literals of itself the byte
    carries (0, 1, 2) and the length of the match that ends with it (0: none) — the header's token rule by position."""
    i = np.arange(b.shape[0])
    start = i % segment_bytes == 0
    start[1:] |= b[1:] != b[:-1]
    last = np.append(start[1:], True)
    k = i - np.maximum.accumulate(np.where(start, i, 0))                          # the byte's place in its run
    r = k % PNG_MAX_MATCH
    match = np.where((k > 0) & (r == 0), PNG_MAX_MATCH, np.where((k > 0) & last & (r >= 3), r, 0))
    literals = np.where(k == 0, 1, np.where(last & (r > 0) & (r < 3), r, 0))
    return literals, match


def _png_counts_numpy(b, segment_bytes):
    """int64 [S, PNG_STATS] of one frame's filtered bytes."""
    n = b.shape[0]
    n_seg = -(-n // segment_bytes)
    literals, match = _png_tokens(b, segment_bytes)
    i = np.arange(n)
    seg, on = i // segment_bytes, match > 0
    stats = np.bincount(seg * PNG_STATS + b, weights=literals, minlength=n_seg * PNG_STATS)
    stats += np.bincount(seg[on] * PNG_STATS + _LEN_SYMBOL[match[on]], minlength=n_seg * PNG_STATS)
    stats = stats.astype(np.int64).reshape(n_seg, PNG_STATS)
    stats[:, PNG_SYMBOLS] = np.bincount(seg[on], weights=_LEN_BITS[match[on]], minlength=n_seg)
    stats[:, PNG_SYMBOLS + 1] = np.bincount(seg[on], minlength=n_seg)
    firsts = np.arange(0, n, segment_bytes)
    sizes = np.minimum(segment_bytes, n - firsts)
    stats[:, PNG_SYMBOLS + 2] = np.add.reduceat(b, firsts) % _ADLER
    stats[:, PNG_SYMBOLS + 3] = np.add.reduceat(((sizes[seg] - i % segment_bytes) % _ADLER) * b, firsts) % _ADLER
    return stats


def png_counts(filtered, segment_rows):
    """int32 [F, S, PNG_STATS], S = ceil(H / segment_rows): per segment of ``segment_rows`` filtered rows the number of times every literal/length symbol is
    coded ([256], end of block, stays 0: it comes once a segment), at [286] the matches' extra bits, at [287] the matches, at [288:290] the Adler pair
    (s1 = sum b, s2 = sum (L - i) b_i, mod 65521).  The token rule is p3d_video.h's: runs of equal bytes, a literal, then matches at distance 1 of up to
    258.  Device tensors: ONE ``p3d_video_png_count`` launch, no synchronisation; CPU tensors: the numpy formulation."""
    f, h, r = _check_filtered(filtered, 'png_counts')
    rows = min(_check_segment_rows(segment_rows), max(h, 1))
    n_seg = -(-h // rows)
    if f * h == 0 or r <= 1:
        return torch.zeros([f, n_seg, PNG_STATS], dtype=torch.int32, device=filtered.device)
    filtered = filtered.contiguous()
    if not filtered.is_cuda:
        return torch.from_numpy(np.stack([_png_counts_numpy(x.reshape(-1).to(torch.int64).numpy(), rows * r) for x in filtered]).astype(np.int32))
    stats = torch.empty([f, n_seg, PNG_STATS], dtype=torch.int32, device=filtered.device)
    with _lib.kernel_timer('video_png_count', stats):
        code = video_lib().p3d_video_png_count(_lib.ptr(filtered), f, h, r, rows, _lib.ptr(stats), _lib.stream_of(stats))
    _check(code, 'video_png_count')
    return stats


def png_code_lengths(counts, limit=15):
    """int64 [n]: the code length of every symbol of the histogram ``counts`` [n] (0 for an unused one) — an optimal prefix code among those of at most
    ``limit`` bits, by package-merge.  The used symbols are ordered by (count, symbol); ``limit`` times, the list of the level below is paired up into
    packages and merged with the symbols by weight, a symbol before a package of its weight; the lightest 2 u - 2 items of the top list are taken (u used
    symbols), and a symbol's length is the number of levels at which it is taken — at every level a prefix of the ordered symbols, so only their number is
    tracked.  One used symbol gets one bit, none gets nothing.  ValueError when 2^limit codes are too few."""
    counts = np.asarray(torch.as_tensor(counts).cpu() if torch.is_tensor(counts) else counts, dtype=np.int64).reshape(-1)
    if (counts < 0).any():
        raise ValueError('png_code_lengths: counts must be >= 0')
    lengths = np.zeros(counts.shape[0], dtype=np.int64)
    order = np.flatnonzero(counts)
    order = order[np.argsort(counts[order], kind='stable')]                       # by (count, symbol)
    u = order.shape[0]
    if u > 1 << int(limit):
        raise ValueError(f'png_code_lengths: {u} symbols do not fit {limit} bits')
    if u <= 1:
        lengths[order] = 1
        return lengths
    weights = counts[order]
    is_symbol = np.ones(u, dtype=bool)
    level_w, levels = weights, [is_symbol]
    for _ in range(int(limit) - 1):
        pairs = level_w.shape[0] // 2
        both = np.concatenate([weights, level_w[0:2 * pairs:2] + level_w[1:2 * pairs:2]])
        by_weight = np.argsort(both, kind='stable')                               # the symbols stand first: they win ties
        level_w = both[by_weight]
        levels.append(by_weight < u)
    need, by_rank = 2 * u - 2, np.zeros(u, dtype=np.int64)
    for symbols in reversed(levels):
        taken = int(symbols[:need].sum())
        by_rank[:taken] += 1
        need = 2 * (min(need, symbols.shape[0]) - taken)
    lengths[order] = by_rank
    return lengths


def png_canonical_codes(lengths):
    """int64 [n]: the canonical code of every symbol as RFC 1951 section 3.2.2 assigns it from the code ``lengths`` — codes of one length count up in symbol
    order, the first of a length is (the first of the length before + their number) << 1.  A symbol of length 0 has no code (0)."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    per_length = np.bincount(lengths, minlength=2)
    per_length[0] = 0
    codes, code = np.zeros_like(lengths), 0
    for bits in range(1, per_length.shape[0]):
        code = (code + int(per_length[bits - 1])) << 1
        of_length = np.flatnonzero(lengths == bits)
        codes[of_length] = code + np.arange(of_length.shape[0])
    return codes


def _reversed(codes, lengths):
    """Every code with its ``lengths`` bits in reverse order: what a deflate stream, packed from the low bit on, takes."""
    codes, out = np.asarray(codes, dtype=np.int64), np.zeros_like(np.asarray(codes, dtype=np.int64))
    for bit in range(int(np.max(lengths, initial=0))):
        out |= np.where(lengths > bit, ((codes >> bit) & 1) << (lengths - 1 - bit).clip(min=0), 0)
    return out


def png_block_header(lengths):
    """``(bits, n)``: the header of a dynamic-Huffman deflate block for the literal/length code ``lengths`` [286] and the constant distance code (symbols 0 and
    1, one bit each), WITHOUT its BFINAL bit, as an int whose bit i is the i-th bit of the stream, and their number.  BTYPE = 10; HLIT = (the last used symbol
    + 1, at least 257) - 257; HDIST = 1; the lengths of both codes in one sequence, run-length coded by this greedy rule, from the front: a run of zeros of
    11 or more gives 18 with up to 138 of them, of 3 .. 10 gives 17, a shorter one a plain 0; any other length is written once and, while 3 or more equal
    ones follow, 16 with up to 6 of them.  The code-length code over what that used is ``png_code_lengths`` at a limit of 7 bits (a lone symbol gets a
    partner of length 1, so the code is complete), HCLEN trims the unused tail of its fixed order."""
    lengths = [int(v) for v in np.asarray(lengths).reshape(-1)]
    if len(lengths) != PNG_SYMBOLS or not all(0 <= v <= 15 for v in lengths):
        raise ValueError(f'png_block_header: lengths must be {PNG_SYMBOLS} values 0 .. 15')
    n_lit = max(257, max((s + 1 for s, v in enumerate(lengths) if v), default=0))
    sequence = lengths[:n_lit] + [1, 1]
    symbols, i = [], 0                                                            # (symbol, extra bits, extra value)
    while i < len(sequence):
        v, run = sequence[i], 1
        while i + run < len(sequence) and sequence[i + run] == v:
            run += 1
        if v == 0 and run >= 11:
            take = min(run, 138)
            symbols.append((18, 7, take - 11))
        elif v == 0 and run >= 3:
            take = run
            symbols.append((17, 3, take - 3))
        else:
            take = 1
            symbols.append((v, 0, 0))
            while v and run - take >= 3:
                more = min(run - take, 6)
                symbols.append((16, 2, more - 3))
                take += more
        i += take
    used = np.bincount([s for s, _, _ in symbols], minlength=19)
    cl_lengths = png_code_lengths(used, limit=7)
    if (used > 0).sum() == 1:
        cl_lengths[0 if used[0] == 0 else 18] = 1
    cl_codes = _reversed(png_canonical_codes(cl_lengths), cl_lengths)
    n_cl = max(4, max(j + 1 for j, s in enumerate(_CL_ORDER) if cl_lengths[s]))
    bits, n = 0, 0

    def put(value, count):
        nonlocal bits, n
        bits |= int(value) << n
        n += int(count)
    put(2, 2)
    put(n_lit - 257, 5)
    put(1, 5)
    put(n_cl - 4, 4)
    for s in _CL_ORDER[:n_cl]:
        put(cl_lengths[s], 3)
    for s, extra_bits, extra in symbols:
        put(cl_codes[s], cl_lengths[s])
        put(extra, extra_bits)
    return bits, n


class _PngPlan:
    """What the host makes of ONE frame's counts ``stats`` int64 [S, PNG_STATS] and the bytes of its segments ``sizes`` [S]: the code, the block header, the
    bytes every segment takes, and the frame's Adler-32."""

    def __init__(self, stats, sizes):
        n_seg = stats.shape[0]
        counts = stats[:, :PNG_SYMBOLS].sum(axis=0)
        counts[256] = n_seg
        self.lengths = png_code_lengths(counts, 15)
        self.codes = _reversed(png_canonical_codes(self.lengths), self.lengths)
        self.table = (self.lengths << 16 | self.codes).astype(np.uint32)
        self.header, self.header_bits = png_block_header(self.lengths)
        bits = 1 + self.header_bits + stats[:, :PNG_SYMBOLS] @ self.lengths + stats[:, PNG_SYMBOLS] + stats[:, PNG_SYMBOLS + 1] + self.lengths[256]
        self.segment_bytes = (bits + 3 + 7) // 8 + 4                                # the empty stored block after it
        self.segment_bytes[-1] = (bits[-1] + 7) // 8
        s1, s2 = 1, 0
        for size, a, b in zip(sizes.tolist(), stats[:, PNG_SYMBOLS + 2].tolist(), stats[:, PNG_SYMBOLS + 3].tolist()):
            s2 = (s2 + size * s1 + b) % _ADLER
            s1 = (s1 + a) % _ADLER
        self.adler = s2 << 16 | s1

    def header_words(self):
        return np.frombuffer(self.header.to_bytes(4 * PNG_HEADER_WORDS, 'little'), dtype=np.uint32)


def _png_segment_numpy(b, literals, match, plan, final, n_bytes):
    """The bytes of ONE segment: its filtered bytes ``b`` int64 and their tokens."""
    lengths, codes = plan.lengths, plan.codes
    value = np.where(literals == 2, codes[b] | codes[b] << lengths[b], np.where(literals == 1, codes[b], 0))
    count = literals * lengths[b]
    on = match > 0
    symbol = _LEN_SYMBOL[match[on]]
    value[on] = codes[symbol] | _LEN_VALUE[match[on]] << lengths[symbol]            # and the distance code, a 0 bit
    count[on] = lengths[symbol] + _LEN_BITS[match[on]] + 1
    bits = np.zeros(8 * n_bytes, dtype=np.uint8)
    bits[0] = final
    bits[1:1 + plan.header_bits] = [(plan.header >> i) & 1 for i in range(plan.header_bits)]
    first = 1 + plan.header_bits + np.cumsum(count) - count
    for bit in range(int(count.max(initial=0))):
        has = count > bit
        bits[first[has] + bit] = (value[has] >> bit) & 1
    at = 1 + plan.header_bits + int(count.sum())
    bits[at:at + lengths[256]] = [(int(codes[256]) >> i) & 1 for i in range(lengths[256])]
    if not final:
        bits[-16:] = 1                                                              # 00 00 FF FF
    return np.packbits(bits, bitorder='little')


def _png_segment_sizes(h, r, rows):
    firsts = np.arange(0, h, rows)
    return np.minimum(rows, h - firsts) * r


def png_deflate(filtered, segment_rows):
    """``(data uint8 [total], offsets int64 [F + 1])``: the zlib stream of every frame of ``filtered`` (``png_filter``'s rows), frame i at
    ``data[offsets[i]:offsets[i + 1]]``; ``data`` on the filtered bytes' device, ``offsets`` on the host.  78 01, then the frame's segments of ``segment_rows``
    rows, each a dynamic-Huffman block of its own under the frame's ONE code (all but the last followed by an empty stored block, so that every segment starts
    on a byte), then the Adler-32.  Device tensors: ``p3d_video_png_count``, the copy of the counts to the host — the ONLY synchronisation —, there one code, one
    block header and the exact byte length of every segment a frame, their upload in one pinned buffer, and ``p3d_video_png_emit``.  CPU tensors: the numpy
    formulation.  No pixel (F H = 0, or rows of the type byte only): no stream, ``offsets`` all 0."""
    f, h, r = _check_filtered(filtered, 'png_deflate')
    rows = min(_check_segment_rows(segment_rows), max(h, 1))
    if f * h == 0 or r <= 1:
        return torch.zeros([0], dtype=torch.uint8, device=filtered.device), torch.zeros([f + 1], dtype=torch.int64)
    filtered = filtered.contiguous()
    stats = png_counts(filtered, rows)
    host = stats.cpu().numpy().astype(np.int64)
    sizes = _png_segment_sizes(h, r, rows)
    n_seg = sizes.shape[0]
    plans = [_PngPlan(s, sizes) for s in host]
    lengths = np.stack([p.segment_bytes for p in plans])                            # [F, S]
    frame_bytes = lengths.sum(axis=1) + 6
    offsets = np.concatenate([[0], np.cumsum(frame_bytes)])
    starts = offsets[:-1, None] + 2 + np.cumsum(lengths, axis=1) - lengths
    if not filtered.is_cuda:
        out = np.zeros(int(offsets[-1]), dtype=np.uint8)
        for i, plan in enumerate(plans):
            b = filtered[i].reshape(-1).to(torch.int64).numpy()
            literals, match = _png_tokens(b, rows * r)
            out[offsets[i]:offsets[i] + 2] = (0x78, 0x01)
            for s in range(n_seg):
                part = slice(s * rows * r, s * rows * r + int(sizes[s]))
                out[starts[i, s]:starts[i, s] + lengths[i, s]] = _png_segment_numpy(b[part], literals[part], match[part], plan, s == n_seg - 1, int(lengths[i, s]))
            out[offsets[i + 1] - 4:offsets[i + 1]] = list(plan.adler.to_bytes(4, 'big'))
        return torch.from_numpy(out), torch.from_numpy(offsets.astype(np.int64))
    parts = [starts.astype(np.int64).reshape(-1), np.stack([p.table for p in plans]).reshape(-1), np.concatenate([p.header_words() for p in plans]),
             np.array([p.header_bits for p in plans], dtype=np.int32), np.array([p.adler for p in plans], dtype=np.uint32)]
    at = np.concatenate([[0], np.cumsum([p.nbytes for p in parts])])                 # the int64 part first: every part stays aligned
    pinned = torch.empty([int(at[-1])], dtype=torch.uint8, pin_memory=True)
    pinned.numpy()[:] = np.concatenate([p.view(np.uint8) for p in parts])
    up = torch.empty([int(at[-1])], dtype=torch.uint8, device=filtered.device)
    up.copy_(pinned, non_blocking=True)                                             # (pinned, so the copy does not wait for the device)
    data = torch.empty([int(offsets[-1])], dtype=torch.uint8, device=filtered.device)
    import ctypes
    where = [ctypes.c_void_p(up.data_ptr() + int(a)) for a in at[:-1]]
    with _lib.kernel_timer('video_png_emit', data):
        code = video_lib().p3d_video_png_emit(_lib.ptr(filtered), f, h, r, rows, where[1], where[2], where[3], where[4], where[0], _lib.ptr(data), data.shape[0],
                                              _lib.stream_of(data))
    _check(code, 'video_png_emit')
    return data, torch.from_numpy(offsets.astype(np.int64))


def _png_chunk(kind, payload):
    import zlib
    return len(payload).to_bytes(4, 'big') + kind + payload + zlib.crc32(kind + payload).to_bytes(4, 'big')


def _palette_bytes(palette):
    pal = torch.as_tensor(palette).detach().cpu()
    if pal.dtype != torch.uint8 or pal.ndim != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= COLORS:
        raise ValueError(f"mode 'P' needs a palette uint8 [n, 3] with 1 <= n <= {COLORS}")
    return pal.contiguous().numpy().tobytes()


def png_header(h, w, mode, palette=None):
    """Everything of a PNG file before its image data: the signature, IHDR (``w``, ``h``, the depth and colour type of ``mode`` — ``PNG_MODES`` —, deflate,
    adaptive filtering, no interlace) and, for mode 'P', PLTE from ``palette`` uint8 [n <= 256, 3]."""
    if mode not in PNG_MODES:
        raise ValueError(f'mode must be one of {", ".join(PNG_MODES)}, got {mode!r}')
    if not (1 <= int(h) < 1 << 31 and 1 <= int(w) < 1 << 31):
        raise ValueError(f'a PNG is 1 .. 2^31 - 1 pixels a side, got {h} x {w}')
    if (mode == 'P') != (palette is not None):
        raise ValueError("a palette goes with mode 'P', and only with it")
    _, colour_type, depth = PNG_MODES[mode]
    out = _PNG_SIGNATURE + _png_chunk(b'IHDR', int(w).to_bytes(4, 'big') + int(h).to_bytes(4, 'big') + bytes([depth, colour_type, 0, 0, 0]))
    return out + (_png_chunk(b'PLTE', _palette_bytes(palette)) if mode == 'P' else b'')


def _png_streams(frames, mode, palette, filter, what):
    """(frames' F, H, W, the mode, the zlib stream of every frame as bytes)."""
    frames = torch.as_tensor(frames)
    if mode is None:
        if not torch.is_tensor(frames) or frames.ndim not in (3, 4) or (frames.ndim == 4 and frames.shape[3] not in (2, 3, 4)):
            raise ValueError(f'{what}: frames must be uint8 [F, H, W] or [F, H, W, 2 .. 4]')
        mode = 'L' if frames.ndim == 3 else {2: 'LA', 3: 'RGB', 4: 'RGBA'}[frames.shape[3]]
    if mode not in PNG_MODES:
        raise ValueError(f'{what}: mode must be one of {", ".join(PNG_MODES)}, got {mode!r}')
    bpp = PNG_MODES[mode][0]
    f, h, w = _check_frames(frames, what, (bpp,))
    if (mode == 'P') != (palette is not None):
        raise ValueError(f"{what}: a palette goes with mode 'P', and only with it")
    if f and (h == 0 or w == 0):
        raise ValueError(f'{what}: a PNG has at least one pixel, got {h} x {w}')
    if f == 0:
        return (f, h, w), mode, []
    filtered = png_filter(frames, (0 if mode == 'P' else PNG_ADAPTIVE) if filter is None else filter)
    data, offsets = png_deflate(filtered, png_segment_rows(w, bpp))
    data, offsets = data.cpu().numpy().tobytes(), offsets.tolist()
    return (f, h, w), mode, [data[offsets[i]:offsets[i + 1]] for i in range(f)]


def encode_png(frames, mode=None, palette=None, filter=None):
    """A list of ``bytes``, one complete PNG file per frame: ``png_header``, one IDAT with the frame's zlib stream, IEND.  Frames uint8, on the device or the host
    (or a numpy array), read in place whatever their pitches: [F, H, W] is 'L', [F, H, W, 2] 'LA', [F, H, W, 3] 'RGB', [F, H, W, 4] 'RGBA' when ``mode`` is None;
    ``mode='P'`` takes [F, H, W] indices with ``palette`` uint8 [n <= 256, 3] (every index below n: not checked, it would take a synchronisation), and
    ``mode='I;16'`` takes [F, H, W, 2] big-endian byte pairs (``depth16``).  ``filter``: see ``png_filter``; None is 'none' for 'P', as the specification
    recommends, and 'adaptive' otherwise.  Lossless: a decoder returns the frames' bytes.  From device frames: three launches (filter, count, emit), ONE
    synchronisation with the host (the segments' counts come down, one code a frame goes up) and ONE device -> host copy, of the compressed bytes.  The
    chunks' CRC-32 is ``zlib.crc32`` on the host over those bytes."""
    (f, h, w), mode, streams = _png_streams(frames, mode, palette, filter, 'encode_png')
    if not streams:
        return []
    header, end = png_header(h, w, mode, palette), _png_chunk(b'IEND', b'')
    return [header + _png_chunk(b'IDAT', s) + end for s in streams]


def save_png(path, frame, mode=None, palette=None, filter=None):
    """One frame — uint8 [H, W] or [H, W, bpp], on the device or the host — as a PNG file (``encode_png``).  Returns its bytes."""
    frame = torch.as_tensor(frame)
    if frame.ndim not in (2, 3):
        raise ValueError(f'save_png: frame must be uint8 [H, W] or [H, W, bpp], got {tuple(frame.shape)}')
    stream, = encode_png(frame[None], mode, palette, filter)
    with open(path, 'wb') as fh:
        fh.write(stream)
    return stream


def save_png_sequence(pattern, frames, mode=None, palette=None, filter=None):
    """Every frame as a PNG file of its own, frame i at ``pattern.format(i)`` (say 'frame_{:04d}.png'), all encoded in one pass of ``encode_png``.  Returns
    the paths."""
    paths = []
    for i, stream in enumerate(encode_png(frames, mode, palette, filter)):
        paths.append(str(pattern).format(i))
        with open(paths[-1], 'wb') as fh:
            fh.write(stream)
    return paths


def save_apng(path, frames, fps=60, loops=0, mode=None, palette=None, filter=None):
    """The frames (``encode_png``'s contract) as an animated PNG: IHDR (and PLTE), acTL (the number of frames; ``loops`` plays, 0 for ever), then per frame fcTL —
    the whole canvas, the delay 1 / ``fps`` as a fraction of 16-bit terms, dispose 0 (none), blend 0 (source) — and its zlib stream, as IDAT for frame 0 (a
    viewer without APNG shows it) and as fdAT after that, fcTL and fdAT sharing one running sequence number.  Every frame is coded whole: bit-exact and
    independent of its neighbours.  ValueError for no frame.  Returns the zlib streams."""
    import fractions
    rate = fractions.Fraction(fps)
    if rate <= 0:
        raise ValueError(f'save_apng: fps must be > 0, got {fps!r}')
    delay = (1 / rate).limit_denominator(65535)
    if delay.numerator > 65535:
        raise ValueError(f'save_apng: a frame of {float(1 / rate)} s does not fit the 16-bit delay')
    if isinstance(loops, bool) or int(loops) != loops or not 0 <= int(loops) < 1 << 31:
        raise ValueError(f'save_apng: loops must be an integer >= 0, got {loops!r}')
    (f, h, w), mode, streams = _png_streams(frames, mode, palette, filter, 'save_apng')
    if f == 0:
        raise ValueError('save_apng: an APNG needs at least one frame')
    out, sequence = [png_header(h, w, mode, palette), _png_chunk(b'acTL', f.to_bytes(4, 'big') + int(loops).to_bytes(4, 'big'))], 0
    for i, s in enumerate(streams):
        control = w.to_bytes(4, 'big') + h.to_bytes(4, 'big') + bytes(8) + delay.numerator.to_bytes(2, 'big') + delay.denominator.to_bytes(2, 'big') + bytes(2)
        out.append(_png_chunk(b'fcTL', sequence.to_bytes(4, 'big') + control))
        sequence += 1
        if i == 0:
            out.append(_png_chunk(b'IDAT', s))
        else:
            out.append(_png_chunk(b'fdAT', sequence.to_bytes(4, 'big') + s))
            sequence += 1
    out.append(_png_chunk(b'IEND', b''))
    with open(path, 'wb') as fh:
        fh.write(b''.join(out))
    return streams


def png_chunks(data):
    """``[(type, payload)]`` of a PNG or APNG file's bytes (or of the file at a path), in order — for tests, and for users without a viewer.  ValueError for a
    wrong signature, a chunk that runs past the end, a CRC-32 that does not match, or bytes after IEND."""
    import zlib
    if not isinstance(data, (bytes, bytearray)):
        with open(data, 'rb') as fh:
            data = fh.read()
    if data[:8] != _PNG_SIGNATURE:
        raise ValueError('png_chunks: not a PNG signature')
    at, chunks = 8, []
    while at < len(data):
        size, kind = int.from_bytes(data[at:at + 4], 'big'), bytes(data[at + 4:at + 8])
        if at + 12 + size > len(data):
            raise ValueError(f'png_chunks: the chunk {kind!r} at {at} runs past the end')
        payload = bytes(data[at + 8:at + 8 + size])
        if zlib.crc32(kind + payload) != int.from_bytes(data[at + 8 + size:at + 12 + size], 'big'):
            raise ValueError(f'png_chunks: the CRC of the chunk {kind!r} at {at} does not match')
        chunks.append((kind, payload))
        at += 12 + size
        if kind == b'IEND' and at != len(data):
            raise ValueError(f'png_chunks: {len(data) - at} bytes after IEND')
    if not chunks or chunks[0][0] != b'IHDR' or chunks[-1][0] != b'IEND':
        raise ValueError('png_chunks: a PNG runs from IHDR to IEND')
    return chunks


def depth16(depth, lo, hi):
    """uint8 [..., 2]: float ``depth`` as the big-endian byte pairs of 16-bit samples, mode 'I;16' of ``encode_png`` — clamp(floor((d - lo) / (hi - lo) 65535 +
    0.5), 0, 65535) in fp64 torch ops on the depth's device; no kernel of this package, no synchronisation.  NaN becomes 0."""
    depth = torch.as_tensor(depth)
    if not float(hi) > float(lo):
        raise ValueError(f'depth16: hi must be above lo, got {lo!r} .. {hi!r}')
    v = torch.floor((depth.to(torch.float64) - float(lo)) / (float(hi) - float(lo)) * 65535 + 0.5)
    v = torch.nan_to_num(v, nan=0.0).clamp(0, 65535).to(torch.int64)
    return torch.stack([v >> 8, v & 255], dim=-1).to(torch.uint8)
