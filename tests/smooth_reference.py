"""numpy restatement of the smooth splat (include/dpr.h, SMOOTH SPLAT): forward and all six gradients, any dtype,
batched.  The CPU reference of tests/test_smooth_reference.py and tests/test_smooth_gpu.py.

Shapes (always batched): points (P, N_in), rotation (B, N_out, N_in), translation (B, N_out), background / out_weight
(B,) or None, point_weight (P,) or None; out / ds_dout grid + (B,).
"""
import itertools

import numpy as np


def _terms(grid, points, rotation, translation, dtype):
    """Per pose b: (accepted point indices, j0 (A, N), w (A, N, 3), dw (A, N, 3))."""
    n = np.asarray(grid, dtype=dtype)
    pts = np.asarray(points, dtype=dtype)
    for b in range(rotation.shape[0]):
        R, t = np.asarray(rotation[b], dtype=dtype), np.asarray(translation[b], dtype=dtype)
        coord = ((pts @ R.T + t) + dtype(1)) * (n / dtype(2))
        with np.errstate(invalid="ignore"):
            ok = np.all((coord >= -1) & (coord < n + 1), axis=1)  # (NaN compares false: rejected)
        idx = np.nonzero(ok)[0]
        c = coord[idx]
        f = np.floor(c)
        u = c - (f + dtype(0.5))
        a, bb = dtype(0.5) - u, dtype(0.5) + u
        w = np.stack([a * a / 2, dtype(0.75) - u * u, bb * bb / 2], axis=-1)
        dw = np.stack([-a, -2 * u, bb], axis=-1)
        yield b, idx, f.astype(np.int64), w.astype(dtype), dw.astype(dtype)


def _defaults(B, P, background, out_weight, point_weight, dtype):
    bg = np.zeros(B, dtype) if background is None else np.asarray(background, dtype=dtype).reshape(B)
    ow = np.ones(B, dtype) if out_weight is None else np.asarray(out_weight, dtype=dtype).reshape(B)
    pw = np.ones(P, dtype) if point_weight is None else np.asarray(point_weight, dtype=dtype).reshape(P)
    return bg, ow, pw


def raster_smooth(grid, points, rotation, translation, background=None, out_weight=None, point_weight=None,
                  dtype=np.float64):
    dtype = np.dtype(dtype).type
    grid = tuple(int(g) for g in grid)
    N, B, P = len(grid), rotation.shape[0], points.shape[0]
    bg, ow, pw = _defaults(B, P, background, out_weight, point_weight, dtype)
    out = np.empty(grid + (B,), dtype=dtype)
    for b, idx, j0, w, _dw in _terms(grid, points, rotation, translation, dtype):
        plane = np.full(grid, bg[b], dtype=dtype)
        for s in itertools.product(range(3), repeat=N):
            cell = j0 + (np.asarray(s) - 1)
            inside = np.all((cell >= 0) & (cell < np.asarray(grid)), axis=1)
            v = ow[b] * pw[idx]
            for d in range(N):
                v = v * w[:, d, s[d]]
            np.add.at(plane, tuple(cell[inside].T), v[inside])
        out[..., b] = plane
    return out


def raster_pullback_smooth(ds_dout, points, rotation, translation, out_weight=None, point_weight=None,
                           dtype=np.float64):
    """(ds_dpoints (P, N_in), ds_drotation (B, N_out, N_in), ds_dtranslation (B, N_out), ds_dbackground (B,),
    ds_dout_weight (B,), ds_dpoint_weight (P,))."""
    dtype = np.dtype(dtype).type
    g = np.asarray(ds_dout, dtype=dtype)
    grid = g.shape[:-1]
    N, B, P = len(grid), rotation.shape[0], points.shape[0]
    n_in = points.shape[1]
    _bg, ow, pw = _defaults(B, P, None, out_weight, point_weight, dtype)
    pts = np.asarray(points, dtype=dtype)
    d_pts = np.zeros((P, n_in), dtype)
    d_rot = np.zeros((B, N, n_in), dtype)
    d_trans = np.zeros((B, N), dtype)
    d_ow = np.zeros(B, dtype)
    d_pw = np.zeros(P, dtype)
    d_bg = g.reshape(-1, B).sum(axis=0).astype(dtype)
    n = np.asarray(grid, dtype=dtype)
    for b, idx, j0, w, dw in _terms(grid, points, rotation, translation, dtype):
        W = np.zeros(len(idx), dtype)
        dcoord = np.zeros((len(idx), N), dtype)
        for s in itertools.product(range(3), repeat=N):
            cell = j0 + (np.asarray(s) - 1)
            inside = np.all((cell >= 0) & (cell < np.asarray(grid)), axis=1)
            gv = np.zeros(len(idx), dtype)
            gv[inside] = g[..., b][tuple(cell[inside].T)]
            prod = gv.copy()
            for d in range(N):
                prod = prod * w[:, d, s[d]]
            W += prod
            for k in range(N):
                term = gv * dw[:, k, s[k]]
                for d in range(N):
                    if d != k:
                        term = term * w[:, d, s[d]]
                dcoord[:, k] += term
        scaled = dcoord * (ow[b] * pw[idx])[:, None] * (n / dtype(2))
        R = np.asarray(rotation[b], dtype=dtype)
        d_trans[b] = scaled.sum(axis=0)
        d_rot[b] = scaled.T @ pts[idx]
        d_pts[idx] += scaled @ R
        d_ow[b] = (W * pw[idx]).sum()
        d_pw[idx] += W * ow[b]
    return d_pts, d_rot, d_trans, d_bg, d_ow, d_pw
