"""Shared by test_edit_host.py / test_edit_gpu.py: the numpy oracle of the stroke rule (a plain per-stroke loop in int64), seeded stroke tables, label maps,
forward-hook counters and the module route of the label entry."""
import numpy as np
import torch


def oracle_paint(base, strokes):
    """base uint8 [H, W], strokes [(x0, y0, x1, y1, t, label)] -> uint8 [H, W]: every stroke in turn, int64 throughout.  A stroke is evaluated on the rows and
    columns within t (twice the capsule's radius) of its endpoints' box; no pixel outside can be covered."""
    out = np.array(base, dtype=np.uint8, copy=True)
    h, w = out.shape
    for x0, y0, x1, y1, t, label in np.asarray(strokes, np.int64).reshape(-1, 6):
        xa, xb, ya, yb = max(min(x0, x1) - t, 0), min(max(x0, x1) + t, w - 1), max(min(y0, y1) - t, 0), min(max(y0, y1) + t, h - 1)
        if xa > xb or ya > yb:
            continue
        ys, xs = np.mgrid[ya:yb + 1, xa:xb + 1].astype(np.int64)
        dx, dy = x1 - x0, y1 - y0
        px, py = xs - x0, ys - y0
        big_l, s = dx * dx + dy * dy, px * dx + py * dy
        cross = px * dy - py * dx
        at_a = 4 * (px * px + py * py) <= t * t
        at_b = 4 * ((px - dx) ** 2 + (py - dy) ** 2) <= t * t
        along = 4 * cross * cross <= t * t * big_l
        out[ya:yb + 1, xa:xb + 1][np.where(s <= 0, at_a, np.where(s >= big_l, at_b, along))] = label
    return out


def float_capsule(h, w, stroke):
    """float64 distance of every pixel to the segment minus t / 2 (negative inside): what the integer rule restates."""
    x0, y0, x1, y1, t, _ = (float(v) for v in stroke)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    dx, dy = x1 - x0, y1 - y0
    big_l = dx * dx + dy * dy
    u = np.clip(((xs - x0) * dx + (ys - y0) * dy) / big_l, 0.0, 1.0) if big_l > 0 else np.zeros_like(xs)
    return np.hypot(xs - (x0 + u * dx), ys - (y0 + u * dy)) - t / 2


def random_strokes(k, h, w, n_labels, seed, t_max=60, margin=40):
    """k strokes with endpoints inside and outside the canvas, thicknesses 1 .. t_max, a few zero-length, a few wholly outside."""
    r = np.random.RandomState(seed)
    s = np.empty([k, 6], np.int64)
    s[:, 0], s[:, 2] = r.randint(-margin, w + margin, k), r.randint(-margin, w + margin, k)
    s[:, 1], s[:, 3] = r.randint(-margin, h + margin, k), r.randint(-margin, h + margin, k)
    short = r.rand(k) < 0.6                                   # brush segments: most strokes are a few pixels long
    s[short, 2] = s[short, 0] + r.randint(-25, 26, int(short.sum()))
    s[short, 3] = s[short, 1] + r.randint(-25, 26, int(short.sum()))
    s[:, 4] = r.randint(1, t_max + 1, k)
    s[:, 5] = r.randint(0, n_labels, k)
    s[::17, 2:4] = s[::17, 0:2]                               # discs
    s[5::31, 0:4] = np.array([-300, -200, -250, -220])        # off the canvas
    s[3::29, 4] = 1                                           # hairlines
    return s


def random_mask(n, h, w, n_labels, seed):
    """uint8 [n, h, w]: blocky regions of every label."""
    r = np.random.RandomState(seed)
    coarse = r.randint(0, n_labels, [n, (h + 7) // 8, (w + 7) // 8]).astype(np.uint8)
    return torch.from_numpy(np.repeat(np.repeat(coarse, 8, axis=1), 8, axis=2)[:, :h, :w].copy())


def fromrgb_layer(n_labels, channels=64, seed=0):
    """The Encoder's first layer with seeded weights and a non-zero bias."""
    from pix2pix3d_amd.training.networks_stylegan2 import Conv2dLayer
    g = torch.Generator().manual_seed(seed)
    layer = Conv2dLayer(n_labels, channels, kernel_size=1, activation='lrelu').eval().requires_grad_(False)
    layer.weight.copy_(torch.randn(layer.weight.shape, generator=g))
    layer.bias.copy_(torch.randn(layer.bias.shape, generator=g))
    return layer


def module_features(layer, mask, n_labels):
    """``fromrgb(one_hot(mask).float())`` on the CPU — the route ``G.mapping`` takes; bytes >= n_labels are an all-zero pixel."""
    m = mask.long()
    hot = torch.nn.functional.one_hot(m.clamp(max=n_labels), n_labels + 1)[..., :n_labels]
    with torch.no_grad():
        return layer(hot.permute(0, 3, 1, 2).float())


class Counters:
    """Forward-hook counters on the Encoder, the mapping MLP's layers and the backbone's synthesis network."""

    def __init__(self, G):
        m = G.backbone.mapping
        self.count = dict(encoder=0, mlp=0, backbone=0)
        fcs = [getattr(m, f'fc{i}') for i in range(m.num_layers)]
        self.n_fc = len(fcs)
        self.handles = [m.embed_mask.register_forward_hook(lambda *a: self._bump('encoder')), G.backbone.synthesis.register_forward_hook(lambda *a: self._bump('backbone'))]
        self.handles += [fc.register_forward_hook(lambda *a: self._bump('mlp')) for fc in fcs]

    def _bump(self, key):
        self.count[key] += 1

    def take(self):
        """(Encoder passes, MLP passes, backbone passes) since the last call."""
        c, self.count = self.count, dict(encoder=0, mlp=0, backbone=0)
        assert c['mlp'] % self.n_fc == 0
        return c['encoder'], c['mlp'] // self.n_fc, c['backbone']

    def remove(self):
        for h in self.handles:
            h.remove()


def demo_pose(G):
    from pix2pix3d_amd import configs
    rk = G.rendering_kwargs
    return configs.orbit_camera(9, radius=rk['avg_camera_radius'], pivot=rk['avg_camera_pivot'])
