"""Agreement metrics: how faithfully a generated label map (or edge map) follows the map it was conditioned on — the mIoU and pixel accuracy the pix2pix3D
paper reports for every model, a boundary F-score, and for edge generators the same boundary measures between two ink maps.  The reference has no code for
these (its ``metrics/`` folder measures realism and needs a feature network).

Three primitives with integer rules (csrc/regions/p3d_regions.h states them; the kernels live in libp3d_regions.so beside the region tools and are called
through ``regions.regions_lib()``), each with a torch formulation that CPU tensors take — the definition — and a device kernel whose bytes equal it:

    confusion(truth, pred, n_labels, valid)            int64 [C * C + 1]: counts[t * C + p], and in the last slot the pixels left out
    boundary(mask)                                     uint8 [H, W]: the label where a 4-neighbour differs, 255 elsewhere
    distance_histogram(from_map, sites, nearest, bins) int64 [bins + 2]: squared distances d^2 of the set's pixels to ``nearest``'s sites

Every counter ACCUMULATES into the caller's zeroed int64 tensor (``out``) without a host synchronisation; ``metrics_from_confusion`` /
``metrics_from_boundary`` do the one host read and the fp64 divisions.  ``boundary_counts`` / ``ink_counts`` compose the primitives with ``regions.nearest``,
``Agreement`` accumulates over a dataset, ``evaluate_generator`` runs a generator over (mask or ink, pose) items, and ``EditSession.agreement`` /
``SketchSession.agreement`` measure the current frame against the current canvas.

Launches of libp3d_regions.so (``regions.launch_count()``): ``confusion`` 1 (0 for no frames), ``boundary`` 1, ``distance_histogram`` 1, ``regions.nearest`` 2;
``boundary_counts`` per frame 2 + 2 * 2 + 2 = 8, with ``per_class`` 2 + C * (2 * 2 + 2) = 2 + 6 C; ``ink_counts`` 2 * 2 + 2 = 6."""
import ctypes
import math

import torch

from . import _lib, regions
from .edit import MAX_SIZE

_C = regions.HEADER.constants                           # p3d_regions.h states the bounds
MAX_LABELS, MAX_BINS, MAX_FRAMES = _C['P3D_LABEL_MAX_LABELS'], _C['P3D_LABEL_MAX_BINS'], _C['P3D_LABEL_MAX_FRAMES']
CLASS_AGNOSTIC = tuple(range(255))                      # the site set of "any boundary pixel" (255 is boundary()'s "none")
BOUNDARY_LAUNCHES, INK_LAUNCHES = 8, 6                   # per frame, of libp3d_regions.so (per_class: 2 + 6 C)


# ---- argument checks ---------------------------------------------------------------------------------------------------------------
def _check_maps(what, *maps):
    """(N, H, W) of uint8 / bool maps [H, W] or [N, H, W] with contiguous pixels and one shape and device; the maps as uint8 [N, H, W] views."""
    first, out = maps[0], []
    for name, m in zip(what, maps):
        if not torch.is_tensor(m) or m.dtype not in (torch.uint8, torch.bool) or m.ndim not in (2, 3):
            raise ValueError(f'{name} must be a uint8 [H, W] or [N, H, W] tensor')
        if tuple(m.shape) != tuple(first.shape) or m.device != first.device:
            raise ValueError(f'{name} is {tuple(m.shape)} on {m.device}, {what[0]} {tuple(first.shape)} on {first.device}: the maps must have one size')
        m = m.view(torch.uint8) if m.dtype == torch.bool else m
        m = m[None] if m.ndim == 2 else m
        n, h, w = m.shape
        if not (1 <= h <= MAX_SIZE and 1 <= w <= MAX_SIZE) or n > MAX_FRAMES:
            raise ValueError(f'{name}: 1 .. {MAX_SIZE} pixels a side and at most {MAX_FRAMES} frames, got {tuple(m.shape)}')
        if (w > 1 and m.stride(2) != 1) or (h > 1 and m.stride(1) < w) or (n > 1 and m.stride(0) < (h - 1) * m.stride(1) + w):
            raise ValueError(f'{name} must have contiguous pixels, rows and frames that do not overlap (strides {m.stride()})')
        out.append(m)
    return tuple(out[0].shape), out


def _check_counter(out, size, device, what):
    if out is None:
        return torch.zeros(size, dtype=torch.int64, device=device)
    if not torch.is_tensor(out) or out.dtype != torch.int64 or tuple(out.shape) != tuple(size) or out.device != device or not out.is_contiguous():
        raise ValueError(f'{what}: out must be a contiguous int64 {list(size)} tensor on {device}')
    return out


def _check_bins(bins):
    if isinstance(bins, bool) or int(bins) != bins or not 1 <= int(bins) <= MAX_BINS:
        raise ValueError(f'bins must be an integer 1 .. {MAX_BINS}, got {bins!r}')
    return int(bins)


def _check_labels(n_labels):
    if isinstance(n_labels, bool) or n_labels is None or int(n_labels) != n_labels or not 1 <= int(n_labels) <= MAX_LABELS:
        raise ValueError(f'n_labels must be an integer 1 .. {MAX_LABELS}, got {n_labels!r}')
    return int(n_labels)


# ---- confusion -----------------------------------------------------------------------------------------------------------------------
def _confusion_torch(truth, pred, n_labels, valid):
    t, p = truth.reshape(-1).long(), pred.reshape(-1).long()
    ok = (t < n_labels) & (p < n_labels)
    if valid is not None:
        ok &= valid.reshape(-1) != 0
    return torch.bincount(torch.where(ok, t * n_labels + p, n_labels * n_labels), minlength=n_labels * n_labels + 1)


def confusion(truth, pred, n_labels, valid=None, out=None):
    """int64 [C * C + 1], C = ``n_labels`` (1 .. 32): ``counts[t * C + p] +=`` the pixels with ``truth == t``, ``pred == p``, both < C and ``valid != 0``;
    ``counts[C * C] +=`` the pixels left out for any of those reasons.  ``truth`` / ``pred`` / the optional ``valid`` (uint8 or bool): [H, W] or [N, H, W] of one
    shape, pitched views included.  ``out``: the caller's counter, accumulated into (default: a fresh zeroed one).  Device tensors: ONE
    ``p3d_label_confusion`` launch (none for N = 0), no host synchronisation; CPU tensors: ``bincount`` of ``t * C + p``."""
    n_labels = _check_labels(n_labels)
    given = (truth, pred) if valid is None else (truth, pred, valid)
    (n, h, w), maps = _check_maps(('truth', 'pred', 'valid'), *given)
    t, p, v = maps[0], maps[1], (maps[2] if valid is not None else None)
    out = _check_counter(out, [n_labels * n_labels + 1], t.device, 'confusion')
    if not t.is_cuda:
        out += _confusion_torch(t, p, n_labels, v)
        return out
    def pitches(m):                                                             # (the stride of a dimension of one entry says nothing: a dense one is passed)
        if m is None:
            return 0, 0
        row = m.stride(1) if h > 1 else w
        return row, (m.stride(0) if n > 1 else h * row)
    with _lib.kernel_timer('label_confusion', out):
        code = regions.regions_lib().p3d_label_confusion(_lib.ptr(t), *pitches(t), _lib.ptr(p), *pitches(p), _lib.ptr(v), *pitches(v), n, h, w, n_labels,
                                                         _lib.ptr(out), _lib.stream_of(out))
    regions._check(code, 'label_confusion')
    return out


def metrics_from_confusion(counts):
    """The one host read of a confusion counter (int64 [C * C + 1]) and its metrics, computed in float64 on the host; a plain dict.  With M the C x C matrix
    (rows: truth), tp_c = M[c, c], T_c = the sum of row c (truth pixels of c), P_c = the sum of column c (predicted pixels of c) and n = the sum of M:

        pixels    n                                    left_out   counts[C * C]
        accuracy  sum_c tp_c / n                       (NaN for n = 0)
        iou[c]    tp_c / (T_c + P_c - tp_c)            (NaN where class c is absent from both maps)
        miou      the mean of iou over the classes present in either map (NaN when there is none)
        fw_iou    sum_c T_c * iou[c] / n               over the classes present in the truth (NaN for n = 0)
        dice[c]   2 tp_c / (T_c + P_c)                 (NaN where class c is absent from both maps)
        matrix    M itself, an int64 CPU tensor [C, C]"""
    if not torch.is_tensor(counts) or counts.dtype != torch.int64 or counts.ndim != 1:
        raise ValueError('metrics_from_confusion: counts must be an int64 [C * C + 1] tensor')
    c = math.isqrt(max(counts.numel() - 1, 0))
    if c < 1 or c * c + 1 != counts.numel():
        raise ValueError(f'metrics_from_confusion: {counts.numel()} counts are no C * C + 1')
    host = counts.cpu()
    m = host[:c * c].reshape(c, c)
    mat = m.double()
    tp, t_n, p_n = mat.diagonal(), mat.sum(dim=1), mat.sum(dim=0)
    n = float(mat.sum())
    nan = float('nan')
    union = t_n + p_n - tp
    present = union > 0
    iou = torch.where(present, tp / union.clamp(min=1), torch.full_like(tp, nan))
    dice = torch.where(present, 2 * tp / (t_n + p_n).clamp(min=1), torch.full_like(tp, nan))
    return {'pixels': int(m.sum()), 'left_out': int(host[-1]), 'accuracy': float(tp.sum()) / n if n else nan, 'iou': iou.tolist(),
            'miou': float(iou[present].mean()) if bool(present.any()) else nan, 'fw_iou': float((t_n * iou)[t_n > 0].sum()) / n if n else nan,
            'dice': dice.tolist(), 'matrix': m.clone()}


# ---- boundary ------------------------------------------------------------------------------------------------------------------------
def _boundary_torch(mask):
    diff = torch.zeros_like(mask, dtype=torch.bool)
    for a, b in regions._neighbour_pairs(mask.shape[0], mask.shape[1], 4):      # shifted compares, both ways
        differ = mask[a] != mask[b]
        diff[a] |= differ
        diff[b] |= differ
    return torch.where(diff, mask, torch.tensor(255, dtype=torch.uint8, device=mask.device))


def boundary(mask):
    """uint8 [H, W], contiguous: ``mask[p]`` where some in-image 4-neighbour of p has a different label, 255 elsewhere (so a pixel labelled 255 is never a
    boundary pixel itself, but counts as different to its neighbours).  ``regions.nearest(boundary(mask), [c])`` is then the nearest boundary pixel of class c,
    ``regions.nearest(boundary(mask), range(255))`` the class-agnostic boundary.  Device tensors: ONE ``p3d_label_boundary`` launch; CPU tensors: shifted
    compares."""
    h, w = regions._check_mask(mask, 'mask')
    if not mask.is_cuda:
        return _boundary_torch(mask)
    out = torch.empty([h, w], dtype=torch.uint8, device=mask.device)
    with _lib.kernel_timer('label_boundary', out):
        code = regions.regions_lib().p3d_label_boundary(_lib.ptr(mask), mask.stride(0), _lib.ptr(out), out.stride(0), h, w, _lib.stream_of(out))
    regions._check(code, 'label_boundary')
    return out


# ---- distance histogram --------------------------------------------------------------------------------------------------------------
def _distance_histogram_torch(from_map, words, nearest, bins):
    h, w = from_map.shape
    dev = from_map.device
    table = torch.tensor([(words[l >> 5] >> (l & 31)) & 1 for l in range(256)], dtype=torch.bool, device=dev)
    q = nearest.long()
    py, px = torch.arange(h, dtype=torch.int64, device=dev)[:, None], torch.arange(w, dtype=torch.int64, device=dev)[None, :]
    d2 = (px - q % w) ** 2 + (py - q // w) ** 2
    slot = torch.where(q < 0, bins + 1, d2.clamp(max=bins))
    return torch.bincount(slot[table[from_map.long()]], minlength=bins + 2)


def distance_histogram(from_map, sites, nearest, bins, out=None):
    """int64 [bins + 2]: for every pixel p = (px, py) of ``from_map`` (uint8 [H, W]) whose label is in the set ``sites``, with q = ``nearest[p]`` = qy * W + qx
    (int32 [H, W], contiguous: ``regions.nearest`` of the OTHER map) and d^2 = (px - qx)^2 + (py - qy)^2: ``hist[d^2] += 1`` for d^2 < bins, ``hist[bins] += 1``
    for d^2 >= bins, ``hist[bins + 1] += 1`` for q < 0 (no site).  ``nearest`` must hold indices < H * W: the device does not check.  ``out``: the caller's
    counter, accumulated into.  Device tensors: ONE ``p3d_label_distance_histogram`` launch, no host synchronisation; CPU tensors: ``bincount``."""
    h, w = regions._check_mask(from_map, 'from_map')
    words, bins = regions.site_words(sites), _check_bins(bins)
    if not torch.is_tensor(nearest) or nearest.dtype != torch.int32 or tuple(nearest.shape) != (h, w) or not nearest.is_contiguous() or nearest.device != from_map.device:
        raise ValueError(f'nearest must be a contiguous int32 [{h}, {w}] tensor on {from_map.device}')
    out = _check_counter(out, [bins + 2], from_map.device, 'distance_histogram')
    if not from_map.is_cuda:
        out += _distance_histogram_torch(from_map, words, nearest, bins)
        return out
    with _lib.kernel_timer('label_distance_histogram', out):
        code = regions.regions_lib().p3d_label_distance_histogram(_lib.ptr(from_map), from_map.stride(0), (ctypes.c_uint32 * 8)(*words), _lib.ptr(nearest), bins,
                                                                  _lib.ptr(out), h, w, _lib.stream_of(out))
    regions._check(code, 'label_distance_histogram')
    return out


# ---- boundary and ink counts -----------------------------------------------------------------------------------------------------------
def _both_ways(map_a, map_b, sites, bins, out):
    """out[0] += the distances of b's site pixels to a's sites (precision of b against a), out[1] += those of a's to b's (recall)."""
    near_a, near_b = regions.nearest(map_a, sites), regions.nearest(map_b, sites)
    distance_histogram(map_b, sites, near_a, bins, out=out[0])
    distance_histogram(map_a, sites, near_b, bins, out=out[1])


def boundary_counts(truth, pred, n_labels=None, bins=65, per_class=False, out=None):
    """int64 [2, bins + 2] (``per_class``: [C, 2, bins + 2], C = ``n_labels``): row 0 the ``distance_histogram`` of the PRED boundary pixels to the nearest
    truth boundary pixel, row 1 that of the TRUTH boundary pixels to the nearest pred boundary pixel.  The boundary of a map is ``boundary(map)``: both sides
    of every label change, any label (``per_class``: the pixels of class c beside another label, against the same in the other map).  ``truth`` / ``pred``
    uint8 [H, W] or [N, H, W] (frames are taken one by one); ``out`` is accumulated into.  Per frame 8 launches of libp3d_regions.so (``per_class``: 2 + 6 C),
    no host synchronisation."""
    bins = _check_bins(bins)
    if per_class:
        n_labels = _check_labels(n_labels)
    (n, h, w), (t, p) = _check_maps(('truth', 'pred'), truth, pred)
    out = _check_counter(out, [n_labels, 2, bins + 2] if per_class else [2, bins + 2], t.device, 'boundary_counts')
    for f in range(n):
        bt, bp = boundary(t[f]), boundary(p[f])
        if per_class:
            for c in range(n_labels):
                _both_ways(bt, bp, (c,), bins, out[c])
        else:
            _both_ways(bt, bp, CLASS_AGNOSTIC, bins, out)
    return out


def metrics_from_boundary(hist, tolerance=2):
    """The one host read of a ``boundary_counts`` / ``ink_counts`` counter (int64 [2, bins + 2]; [C, 2, bins + 2] gives a list of C dicts) and its metrics in
    float64 on the host.  With n_k the sum of row k and within_k the sum of its slots d^2 <= tolerance^2 (``tolerance`` in pixels, tolerance^2 < bins):

        precision  within_0 / n_0     pred-boundary pixels within ``tolerance`` of the truth boundary, over all pred-boundary pixels (NaN for n_0 = 0)
        recall     within_1 / n_1     the same in the other direction
        f_score    2 precision recall / (precision + recall)      (0 where both are 0, NaN where one is NaN)
        chamfer    (mean_0 + mean_1) / 2, mean_k = (sum_{d^2 < bins} hist[k, d^2] sqrt(d^2) + (hist[k, bins] + hist[k, bins + 1]) sqrt(bins)) / n_k: the truncated
                   symmetric mean distance, a pixel past the histogram or without any site counting sqrt(bins); summed in bin order
        pred_pixels, truth_pixels      n_0, n_1"""
    if not torch.is_tensor(hist) or hist.dtype != torch.int64 or hist.ndim not in (2, 3) or hist.shape[-2] != 2 or hist.shape[-1] < 3:
        raise ValueError('metrics_from_boundary: hist must be an int64 [2, bins + 2] or [C, 2, bins + 2] tensor')
    bins = hist.shape[-1] - 2
    t2 = math.floor(float(tolerance) ** 2) if tolerance >= 0 else -1
    if not 0 <= t2 < bins:
        raise ValueError(f'metrics_from_boundary: tolerance^2 must be 0 .. bins - 1 = {bins - 1}, got tolerance {tolerance!r}')
    host = hist.cpu()
    if host.ndim == 3:
        return [_boundary_metrics(h.tolist(), bins, t2) for h in host]
    return _boundary_metrics(host.tolist(), bins, t2)


def _boundary_metrics(rows, bins, t2):
    nan = float('nan')
    ratio, mean, total = [], [], []
    for row in rows:
        n = sum(row)
        acc = 0.0
        for d2 in range(bins):                                                  # in bin order, float64
            acc += row[d2] * math.sqrt(d2)
        acc += (row[bins] + row[bins + 1]) * math.sqrt(bins)
        total.append(n)
        ratio.append(sum(row[:t2 + 1]) / n if n else nan)
        mean.append(acc / n if n else nan)
    p, r = ratio
    f = nan if (math.isnan(p) or math.isnan(r)) else (2 * p * r / (p + r) if p + r > 0 else 0.0)
    return {'precision': p, 'recall': r, 'f_score': f, 'chamfer': (mean[0] + mean[1]) / 2, 'pred_pixels': total[0], 'truth_pixels': total[1]}


def ink_counts(ink_a, ink_b, threshold=128, bins=65, out=None):
    """int64 [2, bins + 2] for two ink maps (uint8 [H, W], 255 = full ink; a the truth, b the prediction): both are binarised (``>= threshold``) into 0 / 1 maps;
    row 0 is the ``distance_histogram`` of b's ink pixels to the nearest ink pixel of a, row 1 that of a's to b's.  6 launches of libp3d_regions.so, no host
    synchronisation."""
    bins = _check_bins(bins)
    if isinstance(threshold, bool) or int(threshold) != threshold or not 1 <= int(threshold) <= 255:
        raise ValueError(f'threshold must be an integer 1 .. 255, got {threshold!r}')
    for name, ink in (('ink_a', ink_a), ('ink_b', ink_b)):
        regions._check_mask(ink, name)
    if tuple(ink_a.shape) != tuple(ink_b.shape) or ink_a.device != ink_b.device:
        raise ValueError(f'ink_b is {tuple(ink_b.shape)} on {ink_b.device}, ink_a {tuple(ink_a.shape)} on {ink_a.device}: the maps must have one size')
    out = _check_counter(out, [2, bins + 2], ink_a.device, 'ink_counts')
    _both_ways((ink_a >= int(threshold)).view(torch.uint8), (ink_b >= int(threshold)).view(torch.uint8), (1,), bins, out)
    return out


def ink_agreement(ink_a, ink_b, threshold=128, tolerance=2, bins=65):
    """``metrics_from_boundary`` of ``ink_counts`` — the edge generators' counterpart of mIoU — with ``ink_a`` / ``ink_b``, the two ink pixel counts."""
    m = metrics_from_boundary(ink_counts(ink_a, ink_b, threshold, bins), tolerance)
    m['ink_a'], m['ink_b'] = m['truth_pixels'], m['pred_pixels']
    return m


# ---- the accumulator -----------------------------------------------------------------------------------------------------------------
class Agreement:
    """Counters on ``device`` for a whole dataset: ``add`` / ``add_ink`` accumulate without a host synchronisation, ``result`` is the only read."""

    def __init__(self, n_labels, device, bins=65):
        self.n_labels, self.bins, self.device = _check_labels(n_labels), _check_bins(bins), torch.device(device)
        cells = self.n_labels * self.n_labels + 1
        self._store = torch.zeros([cells + 4 * (self.bins + 2)], dtype=torch.int64, device=self.device)      # one tensor: one copy to the host
        self.counts = self._store[:cells]
        self.boundary = self._store[cells:cells + 2 * (self.bins + 2)].view(2, self.bins + 2)
        self.ink = self._store[cells + 2 * (self.bins + 2):].view(2, self.bins + 2)
        self.frames = self.ink_frames = 0                                       # host counts of what was added

    def add(self, truth, pred, valid=None, boundary=True):
        """One map or a batch [N, H, W] of label maps: the confusion counts and, with ``boundary``, the class-agnostic boundary counts (``valid`` masks the
        confusion counts only)."""
        confusion(truth, pred, self.n_labels, valid, out=self.counts)
        if boundary:
            boundary_counts(truth, pred, bins=self.bins, out=self.boundary)
        self.frames += 1 if truth.ndim == 2 else int(truth.shape[0])

    def add_ink(self, ink_a, ink_b, threshold=128):
        ink_counts(ink_a, ink_b, threshold, self.bins, out=self.ink)
        self.ink_frames += 1

    def result(self, tolerance=2):
        """The metrics so far, one copy to the host: ``metrics_from_confusion``'s dict plus 'boundary' and 'ink' (``metrics_from_boundary`` dicts), 'frames',
        'ink_frames', 'n_labels' and the integer counters 'boundary_counts' / 'ink_counts'."""
        return self.metrics_of(self._store.cpu(), tolerance)

    def metrics_of(self, host, tolerance=2):
        """``result`` from a host copy of the counters (what the sessions keep beside a frame: a repeated question costs no copy)."""
        cells = self.n_labels * self.n_labels + 1
        b, i = host[cells:cells + 2 * (self.bins + 2)].view(2, -1), host[cells + 2 * (self.bins + 2):].view(2, -1)
        out = metrics_from_confusion(host[:cells])
        out.update(boundary=metrics_from_boundary(b, tolerance), ink=metrics_from_boundary(i, tolerance), boundary_counts=b.clone(), ink_counts=i.clone(),
                   frames=self.frames, ink_frames=self.ink_frames, n_labels=self.n_labels)
        return out

    def host_counters(self):
        """The one copy of every counter to the host (a synchronisation), for ``metrics_of``."""
        return self._store.cpu()


# ---- a generator over a dataset --------------------------------------------------------------------------------------------------------
@torch.no_grad()
def evaluate_generator(G, items, cfg, seed=0, truncation_psi=1, views_per_item=1, jitter='frozen', neural_rendering_resolution=None, tolerance=2, bins=65,
                       trace_passes=2, threshold=128, **synthesis_kwargs):
    """``Agreement.result(tolerance)`` of ``G`` over ``items``, an iterable of (mask or ink, pose [25]).  Per item the mapping runs as the sessions run it
    (``EditSession`` for label generators, ``SketchSession`` for one-channel edge generators: geometry rows from the item, appearance rows from z(seed) under the
    forward-facing conditioning pose), ``G.synthesis`` renders at the ITEM'S OWN pose — the only camera at which the output's map answers the input pixel for
    pixel — and ``views.finish_frames`` makes the label map on the device: ``Agreement.add(mask, label_index)``, or for edge generators
    ``add_ink(ink, sketch.trace(255 - grey frame, passes=trace_passes), threshold)``.  ``views_per_item`` samples are drawn per item, with the seeds ``seed``,
    ``seed + 1``, ...  The generated map and the input must have one size (ValueError otherwise, as ``take_view_as_mask``).  ``jitter`` /
    ``neural_rendering_resolution`` as the sessions'; ``synthesis_kwargs`` go to ``G.synthesis`` (``noise_mode`` defaults to 'const').  Nothing is read back
    before the result."""
    import contextlib
    from . import edit, sketch, views
    labelled = int(getattr(G, 'semantic_channels', 0)) >= 2
    common = dict(cfg=cfg, seed=seed, truncation_psi=truncation_psi, jitter=jitter, hold_texture=False, neural_rendering_resolution=neural_rendering_resolution)
    s = edit.EditSession(G, **common) if labelled else sketch.SketchSession(G, **common)
    total = Agreement(s.n_labels if labelled else 1, s.device, bins)
    kwargs = dict(noise_mode='const')
    kwargs.update(synthesis_kwargs)
    for canvas, pose in items:
        s.load(canvas, pose)
        for v in range(int(views_per_item)):
            s.set_seed(int(seed) + v)
            ws = s.encode()
            found, G._last_planes = G._last_planes, G.backbone_planes(ws, noise_mode=kwargs['noise_mode'])
            try:
                with views._frozen_draws(s._draws[0], s._draws[1]) if s._draws is not None else contextlib.nullcontext():
                    out = G.synthesis(ws, s.camera, neural_rendering_resolution=s.nrr, use_cached_backbone=True, **kwargs)
            finally:
                G._last_planes = found
            frame = s._finish(out)
            if labelled:
                _add_label_frame(total, s.mask, frame['label_index'][0])
            else:
                _add_ink_frame(total, s.canvas, frame['label'][0], threshold, trace_passes)
    return total.result(tolerance)


def _same_size(generated, given, what):
    if tuple(generated.shape) != tuple(given.shape):
        raise ValueError(f'{what}: the rendered map is {tuple(generated.shape)}, the input {tuple(given.shape)}')


def _add_label_frame(total, mask, label_index):
    _same_size(label_index, mask, 'agreement')
    total.add(mask, label_index)


def _add_ink_frame(total, canvas, grey, threshold, trace_passes):
    from . import sketch
    _same_size(grey, canvas, 'agreement')
    total.add_ink(canvas, sketch.trace(255 - grey, passes=trace_passes), threshold)
