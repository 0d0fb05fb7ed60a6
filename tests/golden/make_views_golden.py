"""Writes tests/golden/views_cameras.npz: the 25-float camera labels of the reference's video scripts, from the reference's own
``camera_utils.LookAtPoseSampler`` with the formulas of ``applications/generate_video.py`` (:58-61, 90-93, 120-139), for its four
``--cfg`` values x 120 frames.

Run where a checkout of the reference is available (``P3D_REFERENCE=<checkout> python tests/golden/make_views_golden.py``); like
make_golden.py it imports the reference's modules and never ``pix2pix3d_amd``.  What the script does per cfg, quirks included:
``main`` sends seg2cat / seg2face through ``render_video`` and BOTH edge configurations through ``render_video_edge2cat`` (yaw0 = +3.14/2,
yaw on the sine — ``render_video_edge`` is never called); edge2cat takes the seg branch's ranges and focal length.  Pivot and radius are
``G.rendering_kwargs['avg_camera_pivot' / 'avg_camera_radius']`` of the shipped configurations (train.py:425-461; edge2cat trains on the
AFHQ cats' cameras)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.environ['P3D_REFERENCE'])
from camera_utils import LookAtPoseSampler  # noqa: E402

CFGS = {   # cfg: (pitch_range, yaw_range, focal_length, avg_camera_pivot, avg_camera_radius)
    'seg2cat': (0.25, 0.35, 4.2647, [0, 0, -0.06], 2.7),
    'seg2face': (0.25, 0.35, 4.2647, [0, 0, 0.2], 2.7),
    'edge2cat': (0.25, 0.35, 4.2647, [0, 0, -0.06], 2.7),
    'edge2car': (np.pi / 2, np.pi, 1.7074, [0, 0, 0], 1.7),
}


def labels(pitch_range, yaw_range, focal_length, pivot, radius, num_frames=120):
    intrinsics = torch.tensor([[focal_length, 0, 0.5], [0, focal_length, 0.5], [0, 0, 1]])
    out = []
    for k in range(num_frames):                  # yaw on the sine, pitch on the cosine, pi written as 3.14: render_video and render_video_edge2cat alike
        t = 2 * 3.14 * k / num_frames
        yaw, pitch = 3.14 / 2 + yaw_range * np.sin(t), 3.14 / 2 - 0.05 + pitch_range * np.cos(t)
        cam2world = LookAtPoseSampler.sample(yaw, pitch, torch.tensor(pivot, dtype=torch.float32), radius=radius)
        out.append(torch.cat([cam2world.reshape(-1, 16), intrinsics.reshape(-1, 9)], 1))
    return torch.cat(out).to(torch.float32).numpy()


if __name__ == '__main__':
    rec = {}
    for cfg, (pr, yr, focal, pivot, radius) in CFGS.items():
        rec[cfg] = labels(pr, yr, focal, pivot, radius)
        rec[cfg + '_pivot'] = np.asarray(pivot, np.float32)
        rec[cfg + '_radius'] = np.float32(radius)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'views_cameras.npz')
    np.savez_compressed(path, **rec)
    print(path, {k: v.shape for k, v in rec.items()})
