"""numpy restatement of smooth sampling (include/dpr.h, SMOOTH SAMPLING): forward and the four gradients, any dtype,
batched, on the per-pose terms of tests/smooth_reference.py.  The CPU reference of
tests/test_sample_smooth_reference.py and tests/test_sample_smooth_gpu.py.

Shapes (always batched): image / ds_dimage grid + (B,), points (P, N_in), rotation (B, N_out, N_in), translation
(B, N_out); values / ds_dvalues (P, B).
"""
import itertools

import numpy as np

from tests.smooth_reference import _terms


def _cells(grid, j0, N):
    """For every s in {-1, 0, +1}^N: (s + 1, the cells j0 + s, which of them are in the grid)."""
    for s in itertools.product(range(3), repeat=N):
        cell = j0 + (np.asarray(s) - 1)
        yield s, cell, np.all((cell >= 0) & (cell < np.asarray(grid)), axis=1)


def sample_smooth(image, points, rotation, translation, dtype=np.float64):
    dtype = np.dtype(dtype).type
    img = np.asarray(image, dtype=dtype)
    grid = img.shape[:-1]
    N, B, P = len(grid), rotation.shape[0], points.shape[0]
    values = np.zeros((P, B), dtype)
    for b, idx, j0, w, _dw in _terms(grid, points, rotation, translation, dtype):
        acc = np.zeros(len(idx), dtype)
        for s, cell, inside in _cells(grid, j0, N):
            v = np.zeros(len(idx), dtype)
            v[inside] = img[..., b][tuple(cell[inside].T)]
            for d in range(N):
                v = v * w[:, d, s[d]]
            acc += v
        values[idx, b] = acc
    return values


def sample_smooth_pullback(ds_dvalues, image, points, rotation, translation, dtype=np.float64):
    """(ds_dimage grid + (B,), ds_dpoints (P, N_in), ds_drotation (B, N_out, N_in), ds_dtranslation (B, N_out))."""
    dtype = np.dtype(dtype).type
    img = np.asarray(image, dtype=dtype)
    dv = np.asarray(ds_dvalues, dtype=dtype)
    grid = img.shape[:-1]
    N, B, P = len(grid), rotation.shape[0], points.shape[0]
    n_in = points.shape[1]
    pts = np.asarray(points, dtype=dtype)
    d_img = np.zeros(grid + (B,), dtype)
    d_pts = np.zeros((P, n_in), dtype)
    d_rot = np.zeros((B, N, n_in), dtype)
    d_trans = np.zeros((B, N), dtype)
    n = np.asarray(grid, dtype=dtype)
    for b, idx, j0, w, dw in _terms(grid, points, rotation, translation, dtype):
        plane = np.zeros(grid, dtype)
        dcoord = np.zeros((len(idx), N), dtype)
        for s, cell, inside in _cells(grid, j0, N):
            prod = dv[idx, b].copy()
            for d in range(N):
                prod = prod * w[:, d, s[d]]
            np.add.at(plane, tuple(cell[inside].T), prod[inside])
            gv = np.zeros(len(idx), dtype)
            gv[inside] = img[..., b][tuple(cell[inside].T)]
            for k in range(N):
                term = gv * dw[:, k, s[k]]
                for d in range(N):
                    if d != k:
                        term = term * w[:, d, s[d]]
                dcoord[:, k] += term
        d_img[..., b] = plane
        scaled = dcoord * dv[idx, b][:, None] * (n / dtype(2))
        d_trans[b] = scaled.sum(axis=0)
        d_rot[b] = scaled.T @ pts[idx]
        d_pts[idx] += scaled @ np.asarray(rotation[b], dtype=dtype)
    return d_img, d_pts, d_rot, d_trans
