"""Shared by test_sketch_host.py / test_sketch_gpu.py: seeded pictures and drawings, and plain numpy / flood-fill statements of the rules that owe nothing
to the torch formulations of pix2pix3d_amd/sketch.py."""
import numpy as np
import torch


def scene(h=61, w=83, seed=3):
    """uint8 [h, w, 3]: a bright disc, a box that fades in, a faint box, a ramp and +-3 noise from a fixed seed; the three channels differ a little, so the luma weights matter."""
    r = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    grey = 40.0 + xs * (50.0 / w)                                               # the ramp
    grey[(ys - 0.45 * h) ** 2 + (xs - 0.3 * w) ** 2 <= (0.3 * h) ** 2] = 215    # the bright disc: strong edges
    wedge = (ys >= 6) & (ys < 0.5 * h) & (xs >= 0.6 * w) & (xs < 0.95 * w)
    grey[wedge] += (14 + 3 * (xs - 0.6 * w))[wedge]                            # a box that fades in from the left: its weak edges hang on its strong ones
    grey[(ys >= 0.6 * h) & (ys < h - 5) & (xs >= 0.75 * w) & (xs < w - 5)] += 24                    # and one apart from it: weak edges alone
    rgb = np.stack([grey * 1.0, grey * 0.95 + 4, grey * 1.05 - 6], axis=2) + r.randint(-3, 4, [h, w, 3])
    return torch.from_numpy(np.clip(np.rint(rgb), 0, 255).astype(np.uint8))


def random_grey(h, w, seed):
    """uint8 [h, w]: blocks of 5 x 5 random greys plus fine noise — edges of every direction at every tile position."""
    r = np.random.RandomState(seed)
    coarse = r.randint(0, 256, [(h + 4) // 5, (w + 4) // 5])
    img = np.repeat(np.repeat(coarse, 5, axis=0), 5, axis=1)[:h, :w] + r.randint(-6, 7, [h, w])
    return torch.from_numpy(np.clip(img, 0, 255).astype(np.uint8))


def random_rgb(h, w, seed):
    return torch.stack([random_grey(h, w, seed + k) for k in range(3)], dim=2).contiguous()


def drawing(h=48, w=64):
    """(uint8 [h, w] ink, the number of its 8-connected components): a cross and, apart from it, a diagonal, each one pixel wide, ends inside the image."""
    from pix2pix3d_amd import edit
    strokes = [(8, 20, 40, 20, 1, 255), (24, 6, 24, 36, 1, 255), (44, 10, 60, 42, 1, 255)]
    return edit.paint_strokes(torch.zeros(h, w, dtype=torch.uint8), strokes), 2


def crossing_lines(h, w, step=16):
    """uint8 [h, w] ink: one-pixel lines along and across every ``step`` pixels (through the corners of the kernels' tiles) and two long diagonals."""
    ink = np.zeros([h, w], np.uint8)
    ink[::step, :] = 255
    ink[:, ::step] = 255
    ink[step - 1::step, :] = 255
    for k in range(min(h, w)):
        ink[k, k] = ink[k, w - 1 - k] = 255
    return torch.from_numpy(ink)


def numpy_blur3(ink):
    """np.pad(mode='reflect') (an axis of one pixel repeats it) and nine shifted slices, (sum + 4) // 9."""
    a = np.asarray(ink, np.int64)
    h, w = a.shape
    p = np.pad(a, 1, mode='reflect')
    total = sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return ((total + 4) // 9).astype(np.uint8)


def numpy_resize_nearest(a, r):
    h, w = a.shape
    sy = np.minimum(np.arange(r) * h // r, h - 1)
    sx = np.minimum(np.arange(r) * w // r, w - 1)
    return a[sy][:, sx]


def script_condition(mask_u8, convention):
    """The reference scripts' expressions on the prepared uint8 mask [R, R] -> float32 [1, 1, R, R]."""
    m = torch.from_numpy(np.ascontiguousarray(mask_u8))
    if convention == 'dataset':
        return (-(m.float() / 127.5 - 1))[None, None]                          # generate_video.py:198 on the dataset's mask
    return ((255 - m).float() / 127.5 - 1)[None, None]                         # --input: the file is 255 - ink


def flood_components(on):
    """int [h, w]: 8-connected components of the True pixels by a plain flood fill, numbered from 1; 0 elsewhere."""
    on = np.asarray(on, bool)
    h, w = on.shape
    ids, count = np.zeros([h, w], np.int64), 0
    for y0 in range(h):
        for x0 in range(w):
            if on[y0, x0] and not ids[y0, x0]:
                count += 1
                ids[y0, x0] = count
                stack = [(y0, x0)]
                while stack:
                    y, x = stack.pop()
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            yy, xx = y + dy, x + dx
                            if 0 <= yy < h and 0 <= xx < w and on[yy, xx] and not ids[yy, xx]:
                                ids[yy, xx] = count
                                stack.append((yy, xx))
    return ids, count


def label_components(on):
    """``scipy.ndimage.label`` under the 8-neighbourhood when scipy imports, else the flood fill."""
    try:
        from scipy import ndimage
    except ImportError:
        return flood_components(on)
    return ndimage.label(np.asarray(on, bool), structure=np.ones([3, 3], int))


def numpy_link(classes):
    c = np.asarray(classes)
    ids, count = label_components(c != 0)
    strong = np.zeros(count + 1, bool)
    strong[ids[c == 2]] = True
    strong[0] = False
    return (strong[ids] * 255).astype(np.uint8)


def zhang_suen_deletable(step, code):
    """The conditions as the paper lists them, on P2 .. P9 = N, NE, E, SE, S, SW, W, NW."""
    p2, p3, p4, p5, p6, p7, p8, p9 = ((code >> i) & 1 for i in range(8))
    ring = [p2, p3, p4, p5, p6, p7, p8, p9, p2]
    b = p2 + p3 + p4 + p5 + p6 + p7 + p8 + p9
    a = sum(1 for u, v in zip(ring[:-1], ring[1:]) if (u, v) == (0, 1))
    if not (2 <= b <= 6 and a == 1):
        return False
    if step == 0:
        return p2 * p4 * p6 == 0 and p4 * p6 * p8 == 0
    return p2 * p4 * p8 == 0 and p2 * p6 * p8 == 0


def pitched_view(image, shift, fill=77):
    """``image`` (uint8 [h, w] or [h, w, 3]) as a CPU view at an odd offset inside a larger canvas of other bytes: row pitch (w + 6) pixels, the first pixel
    ``shift`` bytes off."""
    h, w = image.shape[:2]
    c = image.shape[2] if image.ndim == 3 else 1
    store = torch.full([(h + 2) * (w + 6) * c + 8], fill, dtype=torch.uint8)
    canvas = store[shift:shift + (h + 2) * (w + 6) * c].view(h + 2, w + 6, c)
    view = canvas[1:1 + h, 2:2 + w] if image.ndim == 3 else canvas[1:1 + h, 2:2 + w, 0]
    view.copy_(image)
    return view
