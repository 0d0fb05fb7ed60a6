"""What a setting costs, measured where the frames are: the error sums behind MAE, MSE and PSNR, and SSIM, between two clips on their own device.

The frame writers of ``video/`` have knobs — ``colors`` / ``dither`` / ``palette`` of the GIFs, ``quality`` / ``subsampling`` of the JPEGs — and so has the
arithmetic (fp16 heads, bf16x3, ``exact_fp32``).  This module says what one of them does to the picture without a copy of the frames to the host
(csrc/video/p3d_video.h states the rules; the kernels live in libp3d_video.so and are reached through ``clips.video_lib()``):

    error_sums(a, b)                      int64 [F, bpp, 4]: per frame and channel sum |d|, sum d^2, max |d| and the number of samples with d != 0
    ssim_sums(a, b)                       int64 [F, bpp, 2]: the sum of round(q 2^32) over the 11 x 11 windows inside the picture, and their number
    metrics_from_sums(error, ssim, n)     the fp64 divisions, on the host: mae, mse, max, changed, psnr, ssim — overall, per channel and per frame
    compare(a, b)                         both sums and ONE host read
    Quality                               an accumulator over calls, like ``evaluate.Agreement``
    difference_map(a, b)                  uint8 heat frames of |d|

Clips are uint8 [F, H, W, bpp], bpp = 2 .. 4, or [F, H, W] (bpp = 1), of one shape on one device, with contiguous pixels and any row and frame pitch
(``clips.check_frames``): a strided selection of frames and a window of a larger canvas are read in place.  SSIM is Wang et al.'s — Gaussian window of
sigma 1.5, K1 = 0.01, K2 = 0.03, L = 255, valid windows only, every channel on its own — stated in integers (the window as 10-bit weights, the moments
exact, the two constants scaled by 2^40) up to three fp64 operations per window, so the torch formulation here, which CPU tensors take, is the definition
and the device kernel's bytes equal it.  The sums ACCUMULATE into ``out`` when the caller passes one: integer sums, no order, no host synchronisation."""
import math

import numpy as np
import torch

from . import _lib, clips

_C = clips.HEADER.constants
TAPS, SHIFT, C1, C2 = _C['P3D_VIDEO_SSIM_TAPS'], _C['P3D_VIDEO_SSIM_SHIFT'], _C['P3D_VIDEO_SSIM_C1'], _C['P3D_VIDEO_SSIM_C2']
HALO = TAPS - 1
S_BITS = 20                                          # the 2-D weights sum to S = 2^20


def ssim_window():
    """int64 [11]: round(1024 g), g the Gaussian of sigma 1.5 normalised to sum 1 — the literals of p3d_video.h; they sum to 1024."""
    g = np.exp(-((np.arange(TAPS) - TAPS // 2) ** 2) / (2 * 1.5 ** 2))
    return torch.from_numpy(np.round(1024 * g / g.sum()).astype(np.int64))


# ---- error sums ----------------------------------------------------------------------------------------------------------------------------
def _error_sums_torch(a, b, out):
    d = (clips.channels(a).to(torch.int64) - clips.channels(b).to(torch.int64)).abs()
    out[..., 0] += d.sum(dim=(1, 2))
    out[..., 1] += (d * d).sum(dim=(1, 2))
    out[..., 2] = torch.maximum(out[..., 2], d.amax(dim=(1, 2)))
    out[..., 3] += (d != 0).sum(dim=(1, 2))
    return out


def error_sums(a, b, out=None):
    """int64 [F, bpp, 4]: per frame and channel, with d = a - b per sample, sum |d|, sum d^2, max |d| and the number of samples with d != 0.  ``out``: the
    caller's contiguous int64 [F, bpp, 4] on the clips' device, to which the call ADDS (the third slot by a maximum): zero it once, accumulate many calls,
    read once.  Device tensors: ONE ``p3d_video_error_sums`` launch, no synchronisation; CPU tensors: the torch formulation."""
    f, h, w, bpp = clips.check_pair(a, b, 'error_sums')
    out = clips.check_sums(out, [f, bpp, 4], a.device, 'error_sums')
    if f * h * w == 0:
        return out
    if not a.is_cuda:
        return _error_sums_torch(a, b, out)
    with _lib.kernel_timer('video_error_sums', out):
        code = clips.video_lib().p3d_video_error_sums(*clips.pair_args(a, b), _lib.ptr(out), _lib.stream_of(out))
    clips.check(code, 'video_error_sums')
    return out


# ---- SSIM ----------------------------------------------------------------------------------------------------------------------------------
def ssim_moments(a, b):
    """(A, B, Pxx, Pyy, Pxy): int64 [F, H - 10, W - 10, bpp] each, the exact weighted sums of x, y, x^2, y^2 and x y over every window (x from ``a``,
    y from ``b``), by a horizontal then a vertical pass of the 1-D window, as the kernel runs them.  Torch ops on the clips' device."""
    g = ssim_window().tolist()
    x, y = clips.channels(a).to(torch.int64), clips.channels(b).to(torch.int64)
    oh, ow = x.shape[1] - HALO, x.shape[2] - HALO
    out = []
    for q in (x, y, x * x, y * y, x * y):
        rows = sum(g[k] * q[:, :, k:k + ow] for k in range(TAPS))
        out.append(sum(g[k] * rows[:, k:k + oh] for k in range(TAPS)))
    return tuple(out)


def ssim_factors(moments):
    """(n1, n2, d1, d2): the four int64 factors of every window, from ``ssim_moments``: n1 = 2 A B + C1, n2 = 2 (S Pxy - A B) + C2, d1 = A^2 + B^2 + C1,
    d2 = S (Pxx + Pyy) - A^2 - B^2 + C2, with S = 2^20 and C1, C2 the header's constants (6.5025 and 58.5225 times 2^40, rounded)."""
    A, B, pxx, pyy, pxy = moments
    ab, aa_bb = A * B, A * A + B * B
    return 2 * ab + C1, 2 * ((pxy << S_BITS) - ab) + C2, aa_bb + C1, ((pxx + pyy) << S_BITS) - aa_bb + C2


def ssim_values(factors):
    """fp64 q = (n1 n2) / (d1 d2) of every window: four conversions (round to nearest even) and three fp64 operations in that order."""
    n1, n2, d1, d2 = (t.to(torch.float64) for t in factors)
    return (n1 * n2) / (d1 * d2)


def _ssim_torch(a, b, out, maps):
    q = ssim_values(ssim_factors(ssim_moments(a, b)))
    out[..., 0] += torch.round(q * float(1 << SHIFT)).to(torch.int64).sum(dim=(1, 2))
    out[..., 1] += q.shape[1] * q.shape[2]
    return q.to(torch.float32) if maps else None


def ssim_sums(a, b, out=None, maps=False):
    """int64 [F, bpp, 2]: per frame and channel the sum over the (H - 10) x (W - 10) windows of round_half_even(q 2^32), q the window's SSIM, and the number
    of windows; ``H < 11`` or ``W < 11`` has no window and adds nothing.  ``out`` accumulates as ``error_sums``' does.  With ``maps`` the call returns
    ``(sums, map)``, map float32 [F, H - 10, W - 10, bpp] (bpp = 1 included) holding (float) q of every window, for heat maps.  Device tensors: ONE
    ``p3d_video_ssim`` launch, no synchronisation; CPU tensors: the torch formulation (``ssim_moments``, ``ssim_factors``, ``ssim_values``)."""
    f, h, w, bpp = clips.check_pair(a, b, 'ssim_sums')
    out = clips.check_sums(out, [f, bpp, 2], a.device, 'ssim_sums')
    oh, ow = max(h - HALO, 0), max(w - HALO, 0)
    heat = torch.empty([f, oh, ow, bpp], dtype=torch.float32, device=a.device) if maps else None
    if f * oh * ow:
        if not a.is_cuda:
            heat = _ssim_torch(a, b, out, maps)
        else:
            with _lib.kernel_timer('video_ssim', out):
                code = clips.video_lib().p3d_video_ssim(*clips.pair_args(a, b), _lib.ptr(out), _lib.ptr(heat), _lib.stream_of(out))
            clips.check(code, 'video_ssim')
    return (out, heat) if maps else out


# ---- the host read ---------------------------------------------------------------------------------------------------------------------------
def _psnr(mse):
    return float('nan') if math.isnan(mse) else float('inf') if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


def _ratio(n, d):
    return float(n) / float(d) if d else float('nan')


def mean(values):
    """The mean of a list of floats; NaN for an empty one."""
    return sum(values) / len(values) if values else float('nan')


def metrics_from_sums(error, ssim=None, samples=None):
    """A plain dict from ``error_sums``' int64 [F, bpp, 4] (and ``ssim_sums``' [F, bpp, 2]): the ONE copy to the host (both tensors in one) and the fp64
    divisions.  ``samples``: the samples of one frame and channel, H W — the four slots do not count them, so the caller says it (``compare`` does).

    Overall, over all frames and channels: 'mae' = sum |d| / n, 'mse' = sum d^2 / n, 'max', 'changed' (the FRACTION of samples that differ),
    'psnr' = 10 log10(255^2 / mse) — inf for mse = 0, NaN for no sample — and 'ssim': the mean over the channels of sum / (windows 2^32), NaN without a window
    or without ``ssim``.  'channel_mae', ..., 'channel_ssim': the same per channel, lists of bpp; 'frame_mae', ..., 'frame_ssim': per frame, lists of F.
    'frames', 'channels', 'samples' (all of them: F bpp H W) and 'windows' (per channel)."""
    if not torch.is_tensor(error) or error.dtype != torch.int64 or error.ndim != 3 or error.shape[2] != 4:
        raise ValueError('metrics_from_sums: error must be an int64 [F, bpp, 4] tensor (error_sums)')
    f, bpp = error.shape[:2]
    if ssim is not None and (not torch.is_tensor(ssim) or ssim.dtype != torch.int64 or tuple(ssim.shape) != (f, bpp, 2) or ssim.device != error.device):
        raise ValueError(f'metrics_from_sums: ssim must be an int64 [{f}, {bpp}, 2] tensor on {error.device} (ssim_sums)')
    if samples is None or isinstance(samples, bool) or int(samples) != samples or int(samples) < 0:
        raise ValueError(f'metrics_from_sums: samples (of a frame and channel: H W) must be an integer >= 0, got {samples!r}')
    n = int(samples)
    host = (error.reshape(-1) if ssim is None else torch.cat([error.reshape(-1), ssim.reshape(-1)])).cpu()      # the host read
    e = [[[int(v) for v in ch] for ch in fr] for fr in host[:f * bpp * 4].view(f, bpp, 4).tolist()]
    s = [[[int(v) for v in ch] for ch in fr] for fr in host[f * bpp * 4:].view(f, bpp, 2).tolist()] if ssim is not None else [[[0, 0]] * bpp] * f
    scale = float(1 << SHIFT)

    def block(frames_of, channels_of):
        """The metrics of the frames and channels picked."""
        cells = [(i, c) for i in frames_of for c in channels_of]
        total = n * len(cells)
        mse = _ratio(sum(e[i][c][1] for i, c in cells), total)
        per_channel = [_ratio(sum(s[i][c][0] for i in frames_of), sum(s[i][c][1] for i in frames_of) * scale) for c in channels_of]
        return {'mae': _ratio(sum(e[i][c][0] for i, c in cells), total), 'mse': mse, 'max': max([e[i][c][2] for i, c in cells], default=0),
                'changed': _ratio(sum(e[i][c][3] for i, c in cells), total), 'psnr': _psnr(mse), 'ssim': mean(per_channel)}
    out = block(range(f), range(bpp))
    per_channel, per_frame = [block(range(f), [c]) for c in range(bpp)], [block([i], range(bpp)) for i in range(f)]
    for key in ('mae', 'mse', 'max', 'changed', 'psnr', 'ssim'):
        out['channel_' + key] = [m[key] for m in per_channel]
        out['frame_' + key] = [m[key] for m in per_frame]
    out.update(frames=f, channels=bpp, samples=n * f * bpp, windows=sum(s[i][0][1] for i in range(f)) if bpp else 0)
    return out


def compare(a, b):
    """``metrics_from_sums`` of ``error_sums(a, b)`` and ``ssim_sums(a, b)``: two launches and ONE host read from device clips."""
    f, h, w, _ = clips.check_pair(a, b, 'compare')
    return metrics_from_sums(error_sums(a, b), ssim_sums(a, b), samples=h * w)


class Quality:
    """Counters on ``device`` for many clips of ``bpp`` bytes a pixel: ``add`` accumulates without a host synchronisation — the two kernels into fresh per-frame
    counters, torch ops on the device fold those into the totals — and ``result`` is the only read.  The clips may differ in size from call to call."""

    def __init__(self, device, bpp=3):
        if isinstance(bpp, bool) or int(bpp) != bpp or not 1 <= int(bpp) <= 4:
            raise ValueError(f'Quality: bpp must be 1 .. 4, got {bpp!r}')
        self.bpp = int(bpp)
        self._store = torch.zeros([self.bpp * 6], dtype=torch.int64, device=device)          # one tensor: one copy to the host
        self.device = self._store.device                                        # ('cuda' resolved to the current 'cuda:0')
        self.error, self.ssim = self._store[:self.bpp * 4].view(1, self.bpp, 4), self._store[self.bpp * 4:].view(1, self.bpp, 2)
        self.frames = self.samples = 0                                          # host counts of what was added (samples: of one channel)

    def add(self, a, b):
        f, h, w, bpp = clips.check_pair(a, b, 'Quality.add')
        if bpp != self.bpp or a.device != self.device:
            raise ValueError(f'Quality.add: the clips have {bpp} bytes a pixel on {a.device}, the counters {self.bpp} on {self.device}')
        e, s = error_sums(a, b), ssim_sums(a, b)
        self.error[0, :, 2] = torch.maximum(self.error[0, :, 2], e[..., 2].amax(dim=0)) if f else self.error[0, :, 2]
        for k in (0, 1, 3):
            self.error[0, :, k] += e[..., k].sum(dim=0)
        self.ssim[0] += s.sum(dim=0)
        self.frames, self.samples = self.frames + f, self.samples + f * h * w

    def result(self):
        """``metrics_from_sums`` of everything added, as ONE frame ('frame_*' lists have one entry; 'frames' counts the frames added)."""
        out = metrics_from_sums(self.error, self.ssim, samples=self.samples)
        out['frames'] = self.frames
        return out


def difference_map(a, b, gain=1):
    """uint8 [F, H, W, 3] heat frames of the largest |a - b| over a pixel's channels, m = min(gain max_c |d|, 255): black through red (3 m), yellow (3 m - 255
    on green) to white (3 m - 510 on blue), each clamped to 0 .. 255.  Integer torch ops on the clips' device; no kernel of this package, no synchronisation."""
    clips.check_pair(a, b, 'difference_map')
    if isinstance(gain, bool) or int(gain) != gain or int(gain) < 1:
        raise ValueError(f'difference_map: gain must be an integer >= 1, got {gain!r}')
    m = ((clips.channels(a).to(torch.int16) - clips.channels(b).to(torch.int16)).abs().amax(dim=3).to(torch.int32) * int(gain)).clamp(max=255) if a.numel() else \
        torch.zeros(a.shape[:3], dtype=torch.int32, device=a.device)
    return torch.stack([(3 * m).clamp(0, 255), (3 * m - 255).clamp(0, 255), (3 * m - 510).clamp(0, 255)], dim=3).to(torch.uint8)
