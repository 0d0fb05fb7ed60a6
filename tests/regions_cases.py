"""Shared by test_regions_host.py / test_regions_gpu.py: masks with known structure and the first-principles oracles of pix2pix3d_amd.regions (scipy's labelling,
a brute-force nearest site under the (d^2, index) rule)."""
import numpy as np
import torch


def spiral(n, label=3, background=0):
    """uint8 [n, n]: one one-pixel-wide path of ``label`` spiralling inwards from (0, 0), one background pixel between its turns: a single chain of about
    n^2 / 2 pixels under both neighbourhoods (and the background between its turns is a second one)."""
    m = np.full([n, n], background, np.uint8)
    inside = lambda u, v: 0 <= u < n and 0 <= v < n
    x, y, dx, dy = 0, 0, 1, 0
    m[0, 0] = label
    moved = True
    while moved:
        moved = False
        for _ in range(2):                                                     # straight on, else one turn to the right
            nx, ny, ax, ay = x + dx, y + dy, x + 2 * dx, y + 2 * dy
            if inside(nx, ny) and m[ny, nx] == background and (not inside(ax, ay) or m[ay, ax] == background):
                x, y, moved = nx, ny, True
                m[y, x] = label
                break
            dx, dy = -dy, dx
    return torch.from_numpy(m)


def checkerboard(h, w, a=1, b=4):
    ys, xs = np.mgrid[0:h, 0:w]
    return torch.from_numpy(np.where((ys + xs) % 2 == 0, a, b).astype(np.uint8))


def scipy_components(mask, connectivity):
    """int32 [H, W] by ``scipy.ndimage.label`` run per label (cross / full 3 x 3 structure): every pixel gets the smallest linear index of its part."""
    from scipy import ndimage
    mask = np.asarray(mask)
    structure = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)
    out = np.full(mask.shape, -1, np.int64)
    index = np.arange(mask.size).reshape(mask.shape)
    for label in np.unique(mask):
        parts, n = ndimage.label(mask == label, structure=structure)
        smallest = ndimage.minimum(index, parts, np.arange(1, n + 1))
        on = parts > 0
        out[on] = np.asarray(smallest, np.int64)[parts[on] - 1]
    return out.astype(np.int32)


def brute_nearest(mask, sites, radius=-1):
    """int32 [H, W]: for every pixel the site with the smallest (d^2, index), by looking at every site; -1 for none or past the radius."""
    mask = np.asarray(mask)
    h, w = mask.shape
    ys, xs = np.nonzero(np.isin(mask, sorted(sites)))
    out = np.full([h, w], -1, np.int32)
    if len(ys) == 0:
        return out
    py, px = np.mgrid[0:h, 0:w].astype(np.int64)
    d2 = (py[..., None] - ys) ** 2 + (px[..., None] - xs) ** 2               # [H, W, sites]
    key = d2 * (1 << 24) + ys * w + xs
    k = key.argmin(axis=-1)
    best = np.take_along_axis(d2, k[..., None], -1)[..., 0]
    index = (ys * w + xs)[k]
    return np.where((radius < 0) | (best <= radius * radius), index, -1).astype(np.int32)


def disc(r):
    ys, xs = np.mgrid[-r:r + 1, -r:r + 1]
    return ys * ys + xs * xs <= r * r
