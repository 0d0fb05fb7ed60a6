"""Shared by test_views_host.py / test_views_gpu.py: a numpy restatement of the reference scripts' frame finishing, and fp32 test data with the planted
values the arithmetic is pinned on."""
import numpy as np
import torch


def numpy_scale(x, lo, hi):
    """[n, c, h, w] fp32 -> uint8 [n, h, w, c]: ``(clip(x, -1, 1) + 1) * 127.5`` of generate_video.py:65 for any (lo, hi), every step an fp32 numpy operation;
    NaN -> 0 (numpy's own cast of NaN is undefined)."""
    x = np.asarray(x, np.float32)
    s = np.float32(255.0 / (float(hi) - float(lo)))
    t = (x - np.float32(lo)) * s
    assert t.dtype == np.float32
    t = np.where(np.isnan(t), np.float32(0), np.clip(t, np.float32(0), np.float32(255)))
    return t.astype(np.uint8).transpose(0, 2, 3, 1)


def numpy_label(x, palette):
    """[n, c, h, w] fp32, palette uint8 [c, 3] -> (colour uint8 [n, h, w, 3], index uint8 [n, h, w]): argmax over the channels (first maximum; NaN is the
    maximum, first NaN) and the palette loop of training/utils.py:5-15 — one boolean mask and one assignment per label."""
    x = np.asarray(x, np.float32)
    nan = np.isnan(x)
    index = np.where(nan.any(axis=1), nan.argmax(axis=1), np.where(nan, -np.inf, x).argmax(axis=1))
    colour = np.zeros(index.shape + (3,), np.float64)
    for k in range(x.shape[1]):
        colour[index == k] = palette[k]
    return colour.astype(np.uint8), index.astype(np.uint8)


def planted_scale_data(n, c, h, w, seed):
    """Random fp32 overshooting [-1, 1], with exact -1 / 1, NaNs, infinities and the 256 bucket edges k / 127.5 - 1 (and their fp32 neighbours) planted."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, c, h, w, generator=g) * 2.6 - 1.3).to(torch.float32)
    flat = x.reshape(-1)
    k = np.arange(256, dtype=np.float32)
    edges = k / np.float32(127.5) - np.float32(1)
    special = np.concatenate([edges, np.nextafter(edges, np.float32(-2)), np.nextafter(edges, np.float32(2)),
                              np.array([-1, 1, 0, -0.0, np.nan, np.inf, -np.inf, 1.0000001, -1.0000001], np.float32)]).astype(np.float32)
    pos = torch.randperm(flat.numel(), generator=g)[:min(len(special), flat.numel() // 2)]
    flat[pos] = torch.from_numpy(special)[:len(pos)]
    return x


def planted_label_data(n, c, h, w, seed):
    """Random logits with exact ties (between two and between all channels), NaNs (one, several, next to larger values) and infinities planted."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g)
    x = (x * 4).round() / 4                                              # a coarse grid: many natural exact ties
    x[0, :, 0, 0] = 1.5                                                  # all equal -> 0
    x[0, :, 0, 1] = 0.0; x[0, c - 1, 0, 1] = 7.0; x[0, c // 2, 0, 1] = 7.0      # tie of two -> the first
    x[0, :, 0, 2] = 0.0; x[0, c - 1, 0, 2] = float('nan')                # NaN beats everything
    x[0, :, 0, 3] = 0.0; x[0, c - 1, 0, 3] = float('nan'); x[0, c // 2, 0, 3] = float('nan'); x[0, 0, 0, 3] = 99.0      # first NaN
    x[0, :, 0, 4] = float('-inf')                                        # all -inf -> 0
    x[0, :, 0, 5] = 0.0; x[0, c - 1, 0, 5] = float('inf'); x[0, 0, 0, 5] = float('inf')
    x[n - 1, :, h - 1, w - 1] = -3.0; x[n - 1, c - 1, h - 1, w - 1] = -2.75
    return x.to(torch.float32)


def to_device_same_layout(x, device='cuda'):
    """x on the device with the strides AND the storage offset it has on the host (``x.cuda()`` would densify a slice)."""
    whole = torch.as_strided(x, [x.untyped_storage().nbytes() // x.element_size()], [1], 0)
    return torch.as_strided(whole.to(device), x.shape, x.stride(), x.storage_offset())


def _planar(x):
    return x.contiguous()


def _channels_last(x):
    return x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _sliced(x):
    """An interior window of a larger planar tensor with extra channels: no stride is 1-dense, the pointer is offset."""
    n, c, h, w = x.shape
    big = torch.zeros(n, c + 3, h + 2, 2 * w + 5)
    big[:, 1:c + 1, 1:h + 1, 3:3 + 2 * w:2] = x
    return big[:, 1:c + 1, 1:h + 1, 3:3 + 2 * w:2]


_planar.__name__, _channels_last.__name__, _sliced.__name__ = 'planar', 'channels_last', 'sliced'
layouts = [_planar, _channels_last, _sliced]
