"""Region tools on a label map: what an edit script does to REGIONS of the mask (make the eyes larger, remove the ears, move the nose up four pixels,
bucket-fill a hole) where ``edit.paint_strokes`` mirrors a mouse.  The reference's demo has brush strokes only; nothing here has a counterpart there.

Three primitives with integer rules (csrc/regions/p3d_regions.h states them; libp3d_regions.so, a library of its own like the probes'), each with a torch
formulation that CPU tensors take and device kernels whose bytes equal it:

    components(mask, connectivity)          int32 [H, W]: every pixel gets the smallest linear index y * W + x of its component of equal labels
    nearest(mask, sites, radius)            int32 [H, W]: the linear index of the nearest pixel whose label is in ``sites`` by (d^2, index), -1 for none
    warp(mask, region, under, coef)         uint8 [H, W]: the region under an inverse affine map in 1 / 65536 pixel, pasted onto ``under``

and compositions of them in torch element-wise ops on the mask's device, none of which synchronises with the host (``bbox`` does, and says so):
``select``, ``flood_fill``, ``grow``, ``shrink``, ``remove``, ``transform``.  Masks are uint8 [H, W] with contiguous pixels and any row pitch, 1 .. 4096 pixels a
side (``edit._check_mask``); everything is written out of place.  ``EditSession.fill`` / ``grow`` / ``shrink`` / ``remove`` / ``move`` / ``scale`` / ``rotate`` /
``transform`` log these as undo steps (edit.py).  The library also carries the three counting kernels of the agreement metrics (evaluate.py calls them through
``regions_lib()``) and the three kernels of the cross-view warp (reproject.py, likewise): ``HEADER`` declares all nine and ``regions_lib()`` binds them."""
import ctypes
import math

import torch

from . import _lib
from .edit import _check_mask

_side = _lib.SideLibrary('regions')                  # libp3d_regions.so: loaded on the first call, device-guarded; launch_count() is its own counter
REGIONS_LIB_PATH, HEADER = _side.path, _side.header
# bounds of the six warp integers (2^22 and 2^40): c * 4095 stays far inside an int64
MAX_LINEAR, MAX_TRANSLATION = 1 << HEADER.constants['P3D_LABEL_MAX_LINEAR_LOG2'], 1 << HEADER.constants['P3D_LABEL_MAX_TRANSLATION_LOG2']
regions_lib, launch_count, _check = _side.lib, _side.launch_count, _side.check


def site_words(sites):
    """A set of labels as the eight uint32 words of p3d_label_nearest: label l is bit l % 32 of word l // 32."""
    words = [0] * 8
    for label in sites:
        label = int(label)
        if not 0 <= label <= 255:
            raise ValueError(f'site labels must be 0 .. 255, got {label}')
        words[label >> 5] |= 1 << (label & 31)
    return words


# ---- components ----------------------------------------------------------------------------------------------------------------
def _neighbour_pairs(h, w, connectivity):
    """((rows, columns) of a, (rows, columns) of b) for every neighbour offset: a[i] and b[i] are neighbours."""
    pairs = [((slice(0, h), slice(0, w - 1)), (slice(0, h), slice(1, w))), ((slice(0, h - 1), slice(0, w)), (slice(1, h), slice(0, w)))]
    if connectivity == 8:
        pairs += [((slice(0, h - 1), slice(0, w - 1)), (slice(1, h), slice(1, w))), ((slice(0, h - 1), slice(1, w)), (slice(1, h), slice(0, w - 1)))]
    return pairs


def _components_torch(mask, connectivity):
    """Minimum propagation with pointer jumping, until nothing changes: ids[p] is always an index inside p's component, so the fixed point
    (equal over neighbours of one label, ids[ids[p]] == ids[p]) is the smallest index of the component."""
    h, w = mask.shape
    ids = torch.arange(h * w, dtype=torch.int64, device=mask.device).view(h, w)
    pairs = [(a, b, mask[a] == mask[b]) for a, b in _neighbour_pairs(h, w, connectivity)]
    while True:
        new = ids.clone()
        for a, b, same in pairs:
            ia, ib = ids[a], ids[b]
            new[a] = torch.minimum(new[a], torch.where(same, ib, ia))
            new[b] = torch.minimum(new[b], torch.where(same, ia, ib))
        flat = new.view(-1)
        flat = flat[flat]
        new = flat[flat].view(h, w)
        if torch.equal(new, ids):
            return ids.to(torch.int32)
        ids = new


def components(mask, connectivity=4):
    """int32 [H, W], contiguous: a component is a maximal set of equal-label pixels connected under the 4- or 8-neighbourhood; every pixel gets the smallest
    linear index y * W + x of its component — canonical, whatever order the hardware hooks things in.  Device tensors: ``p3d_label_components`` (union-find,
    three launches); CPU tensors: the torch formulation."""
    h, w = _check_mask(mask, 'mask')
    if connectivity not in (4, 8):
        raise ValueError(f'connectivity must be 4 or 8, got {connectivity!r}')
    if not mask.is_cuda:
        return _components_torch(mask, connectivity)
    ids = torch.empty([h, w], dtype=torch.int32, device=mask.device)
    with _lib.kernel_timer('label_components', ids):
        code = regions_lib().p3d_label_components(_lib.ptr(mask), mask.stride(0), _lib.ptr(ids), h, w, connectivity, _lib.stream_of(ids))
    _check(code, 'label_components')
    return ids


# ---- nearest site --------------------------------------------------------------------------------------------------------------------
_NO_KEY = (1 << 63) - 1


def _nearest_torch(mask, words, radius):
    """The two passes of the header.  Pass 2 visits the columns x - k and x + k for growing k and stops once k^2 exceeds every pixel's best d^2 (a host read per
    column offset: this is the CPU formulation; tools/bench_regions.py also times it on device tensors)."""
    h, w = mask.shape
    dev = mask.device
    table = torch.tensor([(words[l >> 5] >> (l & 31)) & 1 for l in range(256)], dtype=torch.bool, device=dev)
    site = table[mask.long()]
    rows = torch.arange(h, dtype=torch.int64, device=dev)[:, None].expand(h, w)
    up = torch.cummax(torch.where(site, rows, -1), dim=0).values                                       # the last site row at or above, -1 for none
    down = torch.flip(torch.cummin(torch.flip(torch.where(site, rows, 1 << 20), [0]), dim=0).values, [0])      # the first site row below or at
    sy = torch.where((up >= 0) & ((rows - up <= down - rows) | (down >= (1 << 20))), up, down)        # the upper one on a tie
    sy = torch.where((up < 0) & (down >= (1 << 20)), -1, sy)
    cols = torch.arange(w, dtype=torch.int64, device=dev)[None, :].expand(h, w)
    best = torch.full([h, w], _NO_KEY, dtype=torch.int64, device=dev)
    kmax = w - 1 if radius < 0 else min(radius, w - 1)
    for k in range(kmax + 1):
        if k * k > int(best.max()) >> 24:
            break
        src, y = sy[:, k:], rows[:, k:]
        key = torch.where(src >= 0, ((k * k + (y - src) ** 2) << 24) | (src * w + cols[:, k:]), _NO_KEY)
        best[:, :w - k] = torch.minimum(best[:, :w - k], key)                                            # the column x + k
        src, y = sy[:, :w - k], rows[:, :w - k]
        key = torch.where(src >= 0, ((k * k + (y - src) ** 2) << 24) | (src * w + cols[:, :w - k]), _NO_KEY)
        best[:, k:] = torch.minimum(best[:, k:], key)                                                    # the column x - k
    found = best != _NO_KEY
    if radius >= 0:
        found &= (best >> 24) <= radius * radius
    return torch.where(found, best & 0xffffff, -1).to(torch.int32)


def nearest(mask, sites, radius=-1):
    """int32 [H, W], contiguous: for every pixel the linear index of the nearest SITE — a pixel whose label is in the set ``sites`` — by squared Euclidean pixel
    distance d^2, ties to the smallest index; a site gets itself; -1 when there is no site or, with ``radius`` >= 0, when d^2 > radius^2 (``radius`` < 0:
    unbounded).  Device tensors: ``p3d_label_nearest`` (two launches: nearest site row per column, then the minimum over columns); CPU tensors: the same two
    passes in torch."""
    h, w = _check_mask(mask, 'mask')
    words, radius = site_words(sites), int(radius)
    if not mask.is_cuda:
        return _nearest_torch(mask, words, radius)
    out = torch.empty([h, w], dtype=torch.int32, device=mask.device)
    workspace = torch.empty([h * w], dtype=torch.int32, device=mask.device)
    with _lib.kernel_timer('label_nearest', out):
        code = regions_lib().p3d_label_nearest(_lib.ptr(mask), mask.stride(0), (ctypes.c_uint32 * 8)(*words), max(-1, min(radius, 1 << 20)),
                                               _lib.ptr(workspace), _lib.ptr(out), h, w, _lib.stream_of(out))
    _check(code, 'label_nearest')
    return out


# ---- warp ----------------------------------------------------------------------------------------------------------------------
def affine_coef(matrix):
    """The six warp integers of a FORWARD 2 x 3 matrix (destination = M [x, y, 1]): its inverse in float64, each coefficient floor(v * 65536 + 0.5).
    ValueError when the matrix is singular, a linear integer exceeds 2^22 in magnitude (a 64-fold reduction) or a translation integer 2^40.  The six
    integers are the definition from then on."""
    m = [[float(v) for v in row] for row in (matrix.tolist() if hasattr(matrix, 'tolist') else matrix)]
    if len(m) != 2 or any(len(row) != 3 for row in m) or not all(math.isfinite(v) for row in m for v in row):
        raise ValueError(f'affine_coef: a finite 2 x 3 matrix is needed, got {matrix!r}')
    (a, b, tx), (c, d, ty) = m
    det = a * d - b * c
    if det == 0.0 or not math.isfinite(det):
        raise ValueError('affine_coef: the matrix is singular')
    inv = [d / det, -b / det, (b * ty - d * tx) / det, -c / det, a / det, (c * tx - a * ty) / det]
    if not all(math.isfinite(v) and abs(v) < 2.0 ** 45 for v in inv):
        raise ValueError('affine_coef: the matrix is singular to working precision')
    coef = tuple(int(math.floor(v * 65536 + 0.5)) for v in inv)
    _check_coef(coef)
    return coef


def _check_coef(coef):
    coef = tuple(int(v) for v in coef)
    if len(coef) != 6:
        raise ValueError(f'warp: coef holds six integers, got {len(coef)}')
    if any(abs(coef[k]) > MAX_LINEAR for k in (0, 1, 3, 4)) or any(abs(coef[k]) > MAX_TRANSLATION for k in (2, 5)):
        raise ValueError(f'warp: coefficients {coef} leave +-2^22 (linear) / +-2^40 (translation)')
    return coef


def _warp_torch(mask, region, under, coef):
    h, w = mask.shape
    px, py = torch.arange(w, dtype=torch.int64, device=mask.device)[None, :], torch.arange(h, dtype=torch.int64, device=mask.device)[:, None]
    qx = (coef[0] * px + coef[1] * py + coef[2] + 32768) >> 16
    qy = (coef[3] * px + coef[4] * py + coef[5] + 32768) >> 16
    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
    sx, sy = qx.clamp(0, w - 1), qy.clamp(0, h - 1)
    return torch.where(inside & (region[sy, sx] != 0), mask[sy, sx], under)


def warp(mask, region, under, coef, out=None):
    """uint8 [H, W]: ``coef`` = six integers (``affine_coef``), the inverse affine map in 1 / 65536 pixel.  For the destination pixel (px, py), with arithmetic shifts,
    qx = (c0 px + c1 py + c2 + 32768) >> 16, qy = (c3 px + c4 py + c5 + 32768) >> 16; out = mask[qy, qx] if q is inside the image and region[qy, qx] != 0,
    else under[py, px].  ``region`` bool / uint8 [H, W]; ``out``: the caller's uint8 [H, W] view (bytes around it stay untouched).  Device tensors: ONE
    ``p3d_label_warp`` launch; CPU tensors: the torch formulation."""
    h, w = _check_mask(mask, 'mask')
    coef = _check_coef(coef)
    region = region.view(torch.uint8) if torch.is_tensor(region) and region.dtype == torch.bool else region
    for t, what in ((region, 'region'), (under, 'under')):
        if _check_mask(t, what) != (h, w) or t.device != mask.device:
            raise ValueError(f'{what} must be uint8 {h} x {w} on {mask.device}')
    if out is None:
        out = torch.empty([h, w], dtype=torch.uint8, device=mask.device)
    elif _check_mask(out, 'out') != (h, w) or out.device != mask.device:
        raise ValueError(f'out must be uint8 {h} x {w} on {mask.device}')
    if out.data_ptr() in (mask.data_ptr(), region.data_ptr(), under.data_ptr()):
        raise ValueError('warp writes out of place: out must not be an input')
    if not mask.is_cuda:
        out.copy_(_warp_torch(mask, region, under, coef))
        return out
    with _lib.kernel_timer('label_warp', out):
        code = regions_lib().p3d_label_warp(_lib.ptr(mask), mask.stride(0), _lib.ptr(region), region.stride(0), _lib.ptr(under), under.stride(0),
                                            _lib.ptr(out), out.stride(0), (ctypes.c_int64 * 6)(*coef), h, w, _lib.stream_of(out))
    _check(code, 'label_warp')
    return out


# ---- compositions: torch element-wise ops on the mask's device, no host synchronisation -------------------------------------------------------------
def _label(label, what='label'):
    if isinstance(label, bool) or int(label) != label or not 0 <= int(label) <= 255:
        raise ValueError(f'{what} must be an integer 0 .. 255, got {label!r}')
    return int(label)


def select(mask, x, y, connectivity=4):
    """bool [H, W]: the component of pixel (x, y)."""
    h, w = _check_mask(mask, 'mask')
    if not (0 <= int(x) < w and 0 <= int(y) < h):
        raise ValueError(f'select: pixel ({x}, {y}) is outside the {h} x {w} mask')
    ids = components(mask, connectivity)
    return ids == ids[int(y), int(x)]


def flood_fill(mask, x, y, label, connectivity=4):
    """``label`` written over the component of pixel (x, y): a bucket fill."""
    return torch.where(select(mask, x, y, connectivity), torch.tensor(_label(label), dtype=torch.uint8, device=mask.device), mask)


def _in_set(mask, labels):
    table = torch.zeros(256, dtype=torch.bool)
    table[[_label(l) for l in labels]] = True
    return table.to(mask.device)[mask.long()]


def grow(mask, label, radius, over=None):
    """Every pixel within ``radius`` (d^2 <= radius^2) of a pixel of ``label`` becomes ``label`` — a dilation by the disc; with ``over`` (a set of labels) only
    pixels whose current label is in it change.  A label that does not occur leaves the mask unchanged."""
    label = _label(label)
    if int(radius) < 0:
        raise ValueError(f'grow: radius must be >= 0, got {radius}')
    change = nearest(mask, {label}, int(radius)) >= 0
    if over is not None:
        change &= _in_set(mask, over)
    return torch.where(change, torch.tensor(label, dtype=torch.uint8, device=mask.device), mask)


def shrink(mask, label, radius):
    """Every pixel of ``label`` within ``radius`` of a pixel of another label takes the label of the nearest such pixel ((d^2, index) order) — an erosion by the
    disc that fills with the surroundings; ``radius`` < 0: every pixel of the label (``remove``).  A mask of that label alone stays unchanged."""
    label = _label(label)
    near = nearest(mask, set(range(256)) - {label}, int(radius))
    taken = mask.reshape(-1)[near.clamp(min=0).long()]
    return torch.where((mask == label) & (near >= 0), taken, mask)


def remove(mask, label):
    """``shrink`` with an unbounded radius: the label disappears under its nearest surroundings."""
    return shrink(mask, label, -1)


def transform(mask, region, matrix, fill='nearest'):
    """The pixels of ``region`` (bool / uint8 [H, W]) moved by the forward 2 x 3 ``matrix`` (or its six ``affine_coef`` integers).  ``under`` is the mask with the
    region vacated: ``fill`` 'nearest' fills it from the nearest pixel outside the region, unbounded (a mask that is all region stays as it is); an int is the
    label it gets.  The result is ``warp(mask, region, under, coef)``."""
    _check_mask(mask, 'mask')
    coef = _check_coef(matrix) if len(matrix) == 6 else affine_coef(matrix)
    region = region != 0
    if isinstance(fill, str):
        if fill != 'nearest':
            raise ValueError(f"transform: fill must be 'nearest' or a label, got {fill!r}")
        near = nearest((~region).view(torch.uint8), {1})                      # the site map is the complement of the region, as a byte map
        under = torch.where(region & (near >= 0), mask.reshape(-1)[near.clamp(min=0).long()], mask)
    else:
        under = torch.where(region, torch.tensor(_label(fill, 'fill'), dtype=torch.uint8, device=mask.device), mask)
    return warp(mask, region.view(torch.uint8), under, coef)


def bbox(region):
    """(x0, y0, x1, y1), inclusive, of the non-zero pixels of ``region`` as four host ints, or None for an empty region.  The one function here that
    SYNCHRONISES with the host (it reads the four numbers back)."""
    if not torch.is_tensor(region) or region.ndim != 2:
        raise ValueError('bbox: region must be a [H, W] tensor')
    on = region != 0
    h, w = on.shape
    cols, rows = on.any(dim=0), on.any(dim=1)
    xs, ys = torch.arange(w, device=on.device), torch.arange(h, device=on.device)
    box = torch.stack([torch.where(cols, xs, w).min(), torch.where(rows, ys, h).min(), torch.where(cols, xs, -1).max(), torch.where(rows, ys, -1).max()]).tolist()
    return None if box[2] < 0 else tuple(int(v) for v in box)
