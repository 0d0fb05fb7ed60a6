"""Shared by test_evaluate_host.py / test_evaluate_gpu.py: the first-principles oracles of pix2pix3d_amd.evaluate in numpy — the confusion matrix by
``np.add.at``, the boundary map by four shifted copies, distances by ``regions_cases.brute_nearest``, and mIoU / accuracy / F by the textbook formulas."""
import numpy as np

from regions_cases import brute_nearest


def oracle_confusion(truth, pred, n_labels, valid=None):
    """int64 [C * C + 1]: one ``np.add.at`` per pixel class, the pixels left out in the last slot."""
    t, p = np.asarray(truth, np.int64).ravel(), np.asarray(pred, np.int64).ravel()
    ok = (t < n_labels) & (p < n_labels)
    if valid is not None:
        ok &= np.asarray(valid).ravel() != 0
    counts = np.zeros(n_labels * n_labels + 1, np.int64)
    np.add.at(counts, t[ok] * n_labels + p[ok], 1)
    counts[-1] = int((~ok).sum())
    return counts


def oracle_boundary(mask):
    """uint8 [H, W]: the label where one of the four shifted copies differs inside the image, 255 elsewhere."""
    m = np.asarray(mask)
    h, w = m.shape
    diff = np.zeros([h, w], bool)
    diff[:, 1:] |= m[:, 1:] != m[:, :-1]
    diff[:, :-1] |= m[:, :-1] != m[:, 1:]
    diff[1:, :] |= m[1:, :] != m[:-1, :]
    diff[:-1, :] |= m[:-1, :] != m[1:, :]
    return np.where(diff, m, 255).astype(np.uint8)


def oracle_histogram(from_map, sites, nearest, bins):
    """int64 [bins + 2] by a loop over the pixels of the set."""
    f, q = np.asarray(from_map), np.asarray(nearest)
    h, w = f.shape
    hist = np.zeros(bins + 2, np.int64)
    for y, x in zip(*np.nonzero(np.isin(f, sorted(sites)))):
        if q[y, x] < 0:
            hist[bins + 1] += 1
        else:
            d2 = (int(x) - int(q[y, x]) % w) ** 2 + (int(y) - int(q[y, x]) // w) ** 2
            hist[min(d2, bins)] += 1
    return hist


def oracle_boundary_counts(truth, pred, sites, bins):
    """int64 [2, bins + 2]: brute-force nearest boundary pixel both ways (row 0: pred against truth, row 1: truth against pred)."""
    bt, bp = oracle_boundary(truth), oracle_boundary(pred)
    return np.stack([oracle_histogram(bp, sites, brute_nearest(bt, sites), bins), oracle_histogram(bt, sites, brute_nearest(bp, sites), bins)])


def textbook_metrics(truth, pred, n_labels):
    """accuracy, per-class IoU and Dice, mIoU over the classes present in either map and frequency-weighted IoU, from boolean masks per class."""
    t, p = np.asarray(truth), np.asarray(pred)
    ok = (t < n_labels) & (p < n_labels)
    iou, dice, fw = [], [], 0.0
    for c in range(n_labels):
        a, b = (t == c) & ok, (p == c) & ok
        inter, union = int((a & b).sum()), int((a | b).sum())
        iou.append(inter / union if union else float('nan'))
        dice.append(2 * inter / (int(a.sum()) + int(b.sum())) if union else float('nan'))
        if a.sum():
            fw += int(a.sum()) * inter / union
    n = int(ok.sum())
    return {'accuracy': int(((t == p) & ok).sum()) / n, 'iou': iou, 'dice': dice, 'miou': float(np.nanmean(iou)), 'fw_iou': fw / n, 'pixels': n}


def textbook_f(hist, tolerance):
    """precision, recall and F from a [2, bins + 2] histogram."""
    hist = np.asarray(hist)
    t2 = int(tolerance * tolerance)
    p, r = (hist[k, :t2 + 1].sum() / hist[k].sum() if hist[k].sum() else float('nan') for k in (0, 1))
    return p, r, (2 * p * r / (p + r) if p + r > 0 else 0.0)
