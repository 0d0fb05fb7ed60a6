"""What a setting costs several octaves down: MS-SSIM (Wang, Simoncelli, Bovik 2003) between two clips on their own device, over a pyramid made there.

Single-scale SSIM (``quality.py``) at 512 x 512 is nearly blind to what separates this package's own variants — blur, ringing and low-frequency colour
shifts of fp16 against fp32 heads, bf16x3 against ``exact_fp32``, 4:2:0 against 4:4:4, ``resample.resize(image_raw)`` against the SR heads — because those
show only at coarser scales.  MS-SSIM weighs the contrast-structure term of four halvings and the full SSIM of the coarsest level, and needs no feature
network (csrc/video/p3d_video.h, "multi-scale frame quality", states the rules; the kernels live in libp3d_video.so and are reached through
``clips.video_lib()``):

    halve(frames, out)                        uint8 [F, H // 2, W // 2(, bpp)]: (s00 + s01 + s10 + s11 + 2) >> 2 per channel, an odd last row or column dropped
    pyramid(frames, levels)                   the list of ``levels`` clips; level 0 is the input itself
    msssim_sums(a, b, levels, out, fused)     int64 [F, bpp, levels, 3]: per frame, channel and level the sum of round(q 2^32), of round(cs 2^32), and the windows
    metrics_from_msssim(sums, weights)        the fp64 work, on the host: per-level means, the weighted product — per frame and channel, per channel, overall
    ms_ssim(a, b, levels, weights)            the sums and ONE host read
    MultiScale                                an accumulator over calls, like ``quality.Quality``
    WEIGHTS, min_size(levels)                 Wang's five exponents; the smallest side ``levels`` levels admit (176 for five)

Clips are ``quality.py``'s: uint8 [F, H, W, bpp], bpp = 2 .. 4, or [F, H, W], of one shape on one device, contiguous pixels and any row and frame pitch
(``clips.check_frames``), read in place.  Per level the window, the moments and the four int64 factors are ``quality.ssim_moments`` / ``ssim_factors``
(on the device: the one window core both kernels run, csrc/video/ssim_window.h): q = (n1 n2) / (d1 d2) as there, cs = n2 / d2 — two conversions and one fp64 division; it may be negative — and a window
contributes round_half_even(q 2^32) and round_half_even(cs 2^32).  So the torch formulation here, which CPU tensors take, is the definition, and the
device kernels' bytes equal it.  A level with a side under 11 has no window: that is an error, never a level skipped.  The pyramid is deliberately NOT
``resample.resize(..., 'box')``, which rounds once per pass.  The sums ACCUMULATE into ``out``: integer sums, no order, no host synchronisation.

Out of scope: luma-only and colour-weighted variants, per-level maps, other window sizes, and bit equality with any float implementation (the test suite
bounds the distance to the textbook float formulation instead)."""
import math

import torch

from . import _lib, clips, quality

_C = clips.HEADER.constants
MAX_LEVELS, TILE_W, TILE_H = _C['P3D_MSSSIM_MAX_LEVELS'], _C['P3D_MSSSIM_TILE_W'], _C['P3D_MSSSIM_TILE_H']
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)   # Wang et al.'s exponents, finest level first
SCALE = float(1 << quality.SHIFT)


def _check_levels(levels, who):
    if isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f'{who}: levels must be an integer in 1 .. {MAX_LEVELS}, got {levels!r}')
    return levels


def min_size(levels=MAX_LEVELS):
    """The smallest side of a clip that ``levels`` levels admit: the last level still holds one 11 x 11 window — 11 * 2^(levels - 1); 176 for five."""
    return quality.TAPS << (_check_levels(levels, 'min_size') - 1)


def _check_size(h, w, levels, who):
    """ValueError for a clip too small for ``levels``; the message names the largest number of levels it admits."""
    if min(h, w) < min_size(levels):
        admits = max([k for k in range(1, MAX_LEVELS + 1) if min(h, w) >= min_size(k)], default=0)
        raise ValueError(f'{who}: {levels} levels need both sides >= {min_size(levels)}, got {h} x {w}, which admits '
                         + (f'levels <= {admits}' if admits else 'no level at all (a side is under 11)'))


def default_weights(levels=MAX_LEVELS):
    """The first ``levels`` of ``WEIGHTS`` rescaled to sum 1."""
    w = WEIGHTS[:_check_levels(levels, 'default_weights')]
    return tuple(v / sum(w) for v in w)


def _check_weights(weights, levels, who):
    if weights is None:
        return default_weights(levels)
    try:
        w = tuple(float(v) for v in weights)
    except (TypeError, ValueError):
        raise ValueError(f'{who}: weights must be {levels} numbers, got {weights!r}')
    if len(w) != levels or not all(math.isfinite(v) and v >= 0 for v in w):
        raise ValueError(f'{who}: weights must be {levels} finite numbers >= 0 (one a level), got {weights!r}')
    return w


# ---- the pyramid ---------------------------------------------------------------------------------------------------------------------------
def _halve_torch(frames):
    nh, nw = frames.shape[1] // 2, frames.shape[2] // 2
    x = frames[:, :2 * nh, :2 * nw].to(torch.int32)
    return ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2] + 2) >> 2).to(torch.uint8)


def halve(frames, out=None):
    """The next level of a clip: uint8 [F, H // 2, W // 2(, bpp)], every sample (s00 + s01 + s10 + s11 + 2) >> 2 over its 2 x 2 block, every channel on its
    own, an odd last row or column dropped; a side of 1 gives an empty level.  ``out``: a clip to write into, any row and frame pitch, apart from
    ``frames`` (``resample.resize``'s rules).  Device tensors: ONE ``p3d_frame_halve`` launch (none for an empty result), no synchronisation; CPU
    tensors: the torch formulation."""
    f, h, w = clips.check_frames(frames, 'halve: frames', bpp=(1, 2, 3, 4))
    out = clips.check_out(out, [f, h // 2, w // 2] + list(frames.shape[3:]), frames, 'halve')
    if out.numel() == 0:
        return out
    if not frames.is_cuda:
        out.copy_(_halve_torch(frames))
        return out
    with _lib.kernel_timer('frame_halve', out):
        code = clips.video_lib().p3d_frame_halve(*clips.clip_args(frames), clips.bpp_of(frames), _lib.ptr(out), out.stride(0), out.stride(1),
                                                 _lib.stream_of(out))
    clips.check(code, 'frame_halve')
    return out


def pyramid(frames, levels=MAX_LEVELS):
    """The list of ``levels`` clips: level 0 is ``frames`` itself (no copy), level k + 1 is ``halve`` of level k.  No size is refused here: a side of 1
    halves to an empty level."""
    clips.check_frames(frames, 'pyramid: frames', bpp=(1, 2, 3, 4))
    out = [frames]
    for _ in range(_check_levels(levels, 'pyramid') - 1):
        out.append(halve(out[-1]))
    return out


# ---- the sums ------------------------------------------------------------------------------------------------------------------------------
def level_values(a, b):
    """(q, cs): fp64 [F, H - 10, W - 10, bpp] each, the two values of every window of one level — q as ``quality.ssim_values``, cs = n2 / d2 (two
    conversions, one division).  Torch ops on the clips' device."""
    factors = quality.ssim_factors(quality.ssim_moments(a, b))
    return quality.ssim_values(factors), factors[1].to(torch.float64) / factors[3].to(torch.float64)


def _level_torch(a, b, out):
    """Adds one level's three sums to ``out`` int64 [F, bpp, 3]."""
    q, cs = level_values(a, b)
    out[..., 0] += torch.round(q * SCALE).to(torch.int64).sum(dim=(1, 2))
    out[..., 1] += torch.round(cs * SCALE).to(torch.int64).sum(dim=(1, 2))
    out[..., 2] += q.shape[1] * q.shape[2]


def _level_device(a, b, sums, level, next_a=None, next_b=None):
    """One ``p3d_frame_msssim_level`` launch: the sums of ``level`` into ``sums`` [F, bpp, levels, 3], the next level into ``next_a`` / ``next_b``."""
    with _lib.kernel_timer(f'frame_msssim_level{level}', sums):
        code = clips.video_lib().p3d_frame_msssim_level(*clips.pair_args(a, b), sums.data_ptr() + level * 3 * sums.element_size(), sums.shape[2] * 3,
                                                        _lib.ptr(next_a), _lib.ptr(next_b), _lib.stream_of(sums))
    clips.check(code, 'frame_msssim_level')


def level_sums(a, b, sums, level, next_a=None, next_b=None):
    """The entry point itself, for callers that bring their own buffers: adds the sums of clips ``a`` and ``b`` — one level — to ``sums[:, :, level]``
    of a contiguous int64 [F, bpp, levels, 3] and, with ``next_a`` and ``next_b`` (contiguous uint8 [F, H // 2, W // 2(, bpp)] on the device), writes the
    next level of both in the same launch.  Device tensors only."""
    f, h, w, bpp = clips.check_pair(a, b, 'level_sums')
    if not a.is_cuda:
        raise ValueError('level_sums: the clips must be on a device (CPU tensors: msssim_sums)')
    if not torch.is_tensor(sums) or sums.dtype != torch.int64 or sums.ndim != 4 or tuple(sums.shape[:2]) != (f, bpp) or sums.shape[3] != 3 \
            or sums.device != a.device or not sums.is_contiguous() or not 0 <= level < sums.shape[2]:
        raise ValueError(f'level_sums: sums must be a contiguous int64 [{f}, {bpp}, levels, 3] tensor on {a.device} with levels > {level}')
    _check_size(h, w, 1, 'level_sums')
    for t in (next_a, next_b):
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.uint8 or tuple(t.shape) != (f, h // 2, w // 2) + tuple(a.shape[3:])
                              or t.device != a.device or not t.is_contiguous()):
            raise ValueError(f'level_sums: next_a and next_b must be contiguous uint8 {[f, h // 2, w // 2] + list(a.shape[3:])} tensors on {a.device}')
    if (next_a is None) != (next_b is None):
        raise ValueError('level_sums: next_a and next_b come together')
    if f:
        _level_device(a, b, sums, level, next_a, next_b)
    return sums


def msssim_sums(a, b, levels=MAX_LEVELS, out=None, fused=True):
    """int64 [F, bpp, levels, 3]: per frame, channel and level the sum over the level's windows of round_half_even(q 2^32), the sum of
    round_half_even(cs 2^32), and the number of windows.  ``out``: the caller's contiguous int64 [F, bpp, levels, 3] on the clips' device, to which the
    call ADDS: zero it once, accumulate many calls, read once.  A clip too small for ``levels`` is a ValueError that names the levels it admits.
    Device tensors, ``fused=True``: ``levels`` launches of ``p3d_frame_msssim_level``, each of which also writes the next level of both clips from the
    samples it has staged; ``fused=False``: ``p3d_frame_halve`` for each clip and level, and the level kernel only measures — 3 levels - 2 launches,
    the same bytes.  No synchronisation either way.  CPU tensors: the torch formulation."""
    f, h, w, bpp = clips.check_pair(a, b, 'msssim_sums')
    _check_levels(levels, 'msssim_sums')
    out = clips.check_sums(out, [f, bpp, levels, 3], a.device, 'msssim_sums')
    _check_size(h, w, levels, 'msssim_sums')
    if f == 0:
        return out
    for k in range(levels):
        last = k == levels - 1
        if not a.is_cuda:
            _level_torch(a, b, out[:, :, k])
            a, b = (a, b) if last else (halve(a), halve(b))
        elif fused and not last:
            shape = [f, a.shape[1] // 2, a.shape[2] // 2] + list(a.shape[3:])
            next_a, next_b = torch.empty(shape, dtype=torch.uint8, device=a.device), torch.empty(shape, dtype=torch.uint8, device=a.device)
            _level_device(a, b, out, k, next_a, next_b)
            a, b = next_a, next_b
        else:
            _level_device(a, b, out, k)
            a, b = (a, b) if last else (halve(a), halve(b))
    return out


# ---- the host read ---------------------------------------------------------------------------------------------------------------------------
def _product(cs, q, weights):
    """prod_{k < L - 1} max(cs_k, 0)^(w_k) * max(q_(L-1), 0)^(w_(L-1)); NaN for a level without a window."""
    terms = list(cs[:-1]) + [q[-1]]
    if any(math.isnan(t) for t in terms):
        return float('nan')
    return math.prod(max(t, 0.0) ** w for t, w in zip(terms, weights))


def metrics_from_msssim(sums, weights=None):
    """A plain dict from ``msssim_sums``' int64 [F, bpp, levels, 3]: the ONE copy to the host and the fp64 work.  ``weights``: ``levels`` exponents >= 0,
    finest level first; default ``default_weights(levels)``, Wang's rescaled to sum 1.

    Per frame, channel and level cs_k = sum / (windows 2^32) and q_k likewise; ms = prod_{k < L - 1} max(cs_k, 0)^(w_k) * max(q_(L-1), 0)^(w_(L-1)).
    'frame_channel_ms_ssim' [F][bpp]; 'channel_ms_ssim' [bpp], the mean over the frames; 'frame_ms_ssim' [F], the mean over the channels; 'ms_ssim',
    the mean over frames and channels of the per-frame values (NaN without a frame).  'level_cs' and 'level_q' [levels]: the means over ALL windows of
    a level, which say at which scale a setting hurts; 'channel_level_cs' / 'channel_level_q' [bpp][levels].  'frames', 'channels', 'levels',
    'weights', and 'windows' [levels] (of one channel)."""
    if not torch.is_tensor(sums) or sums.dtype != torch.int64 or sums.ndim != 4 or sums.shape[3] != 3 or not 1 <= sums.shape[2] <= MAX_LEVELS:
        raise ValueError(f'metrics_from_msssim: sums must be an int64 [F, bpp, levels <= {MAX_LEVELS}, 3] tensor (msssim_sums)')
    f, bpp, levels = sums.shape[:3]
    weights = _check_weights(weights, levels, 'metrics_from_msssim')
    s = sums.cpu().tolist()                                                      # the host read

    def means(cells, slot):
        """Per level: the pooled mean of a slot over the (frame, channel) cells."""
        out = []
        for k in range(levels):
            n = sum(s[i][c][k][2] for i, c in cells)
            out.append(sum(s[i][c][k][slot] for i, c in cells) / (n * SCALE) if n else float('nan'))
        return out
    per = [[_product(means([(i, c)], 1), means([(i, c)], 0), weights) for c in range(bpp)] for i in range(f)]
    everything = [(i, c) for i in range(f) for c in range(bpp)]
    return {'ms_ssim': quality.mean([v for row in per for v in row]), 'frame_channel_ms_ssim': per, 'frame_ms_ssim': [quality.mean(row) for row in per],
            'channel_ms_ssim': [quality.mean([per[i][c] for i in range(f)]) for c in range(bpp)],
            'level_cs': means(everything, 1), 'level_q': means(everything, 0),
            'channel_level_cs': [means([(i, c) for i in range(f)], 1) for c in range(bpp)],
            'channel_level_q': [means([(i, c) for i in range(f)], 0) for c in range(bpp)],
            'frames': f, 'channels': bpp, 'levels': levels, 'weights': list(weights),
            'windows': [sum(s[i][0][k][2] for i in range(f)) if bpp else 0 for k in range(levels)]}


def ms_ssim(a, b, levels=MAX_LEVELS, weights=None):
    """``metrics_from_msssim`` of ``msssim_sums(a, b, levels)``: ``levels`` launches and ONE host read from device clips."""
    _check_weights(weights, _check_levels(levels, 'ms_ssim'), 'ms_ssim')
    return metrics_from_msssim(msssim_sums(a, b, levels), weights)


class MultiScale:
    """Counters on ``device`` for many clips of ``bpp`` bytes a pixel: ``add`` accumulates without a host synchronisation — the kernels into fresh per-frame
    counters, one torch op on the device folds those into the totals — and ``result`` is the only read.  The clips may differ in size from call to call
    (each at least ``min_size(levels)`` a side)."""

    def __init__(self, device, bpp=3, levels=MAX_LEVELS, weights=None):
        if isinstance(bpp, bool) or int(bpp) != bpp or not 1 <= int(bpp) <= 4:
            raise ValueError(f'MultiScale: bpp must be 1 .. 4, got {bpp!r}')
        self.bpp, self.levels = int(bpp), _check_levels(levels, 'MultiScale')
        self.weights = _check_weights(weights, self.levels, 'MultiScale')
        self.sums = torch.zeros([1, self.bpp, self.levels, 3], dtype=torch.int64, device=device)
        self.device = self.sums.device                                          # ('cuda' resolved to the current 'cuda:0')
        self.frames = 0

    def add(self, a, b):
        f, _, _, bpp = clips.check_pair(a, b, 'MultiScale.add')
        if bpp != self.bpp or a.device != self.device:
            raise ValueError(f'MultiScale.add: the clips have {bpp} bytes a pixel on {a.device}, the counters {self.bpp} on {self.device}')
        self.sums[0] += msssim_sums(a, b, self.levels).sum(dim=0)
        self.frames += f

    def result(self):
        """``metrics_from_msssim`` of everything added, as ONE frame: the product of the POOLED per-level means ('frame_*' lists have one entry; 'frames'
        counts the frames added)."""
        out = metrics_from_msssim(self.sums, self.weights)
        out['frames'] = self.frames
        return out
