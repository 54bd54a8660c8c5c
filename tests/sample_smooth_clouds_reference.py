"""numpy restatement of smooth sampling at per-pose clouds (include/dpr.h, SMOOTH SAMPLING, PER-POSE CLOUDS): row b is
tests/sample_smooth_reference.py for (image b, cloud b, pose b).  No arithmetic of its own.  The CPU reference of
tests/test_sample_smooth_clouds_reference.py and tests/test_sample_smooth_clouds_gpu.py.

Shapes: image / ds_dimage grid + (B,), points / ds_dpoints (B, P, N_in), rotation (B, N_out, N_in), translation
(B, N_out); values / ds_dvalues (B, P).
"""
import numpy as np

from tests import sample_smooth_reference as SSR


def sample_smooth_clouds(image, points, rotation, translation, dtype=np.float64):
    img = np.asarray(image)
    B, P = points.shape[0], points.shape[1]
    values = np.zeros((B, P), np.dtype(dtype).type)
    for b in range(B):
        values[b] = SSR.sample_smooth(img[..., b:b + 1], points[b], rotation[b:b + 1], translation[b:b + 1],
                                      dtype=dtype)[:, 0]
    return values


def sample_smooth_clouds_pullback(ds_dvalues, image, points, rotation, translation, dtype=np.float64):
    """(ds_dimage grid + (B,), ds_dpoints (B, P, N_in), ds_drotation (B, N_out, N_in), ds_dtranslation (B, N_out))."""
    img, dv = np.asarray(image), np.asarray(ds_dvalues)
    B = points.shape[0]
    parts = [SSR.sample_smooth_pullback(dv[b][:, None], img[..., b:b + 1], points[b], rotation[b:b + 1],
                                        translation[b:b + 1], dtype=dtype) for b in range(B)]
    t = np.dtype(dtype).type
    if B == 0:
        n_out, n_in = rotation.shape[1], rotation.shape[2]
        return (np.zeros(img.shape, t), np.zeros(points.shape, t), np.zeros((0, n_out, n_in), t),
                np.zeros((0, n_out), t))
    return (np.concatenate([p[0] for p in parts], axis=-1), np.stack([p[1] for p in parts]),
            np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts]))
