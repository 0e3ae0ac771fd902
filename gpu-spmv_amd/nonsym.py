"""nonsym.py — non-symmetric test and benchmark matrices for bicgstab_solve, in numpy only.

Every function returns (n, row_ptrs int32, col_indices int32, values float32) of a square CSR matrix:
* convdiff2d(m, wind) / convdiff3d(m, wind): the 5- / 7-point Laplacian on an m^2 / m^3 grid (diagonal 2 * dims,
  neighbours -1) plus first-order upwind convection: for each axis with wind w >= 0, w is added to the diagonal and
  subtracted from the upstream neighbour (the one at index - 1 along that axis).  `wind` is one value for every
  axis or one per axis.  Non-symmetric for w > 0, a non-singular M-matrix (weakly row diagonally dominant, strictly
  on the boundary, irreducible); columns sorted.
* random_nonsym(n, k, seed, margin, negative_rows): k scattered off-diagonal entries per row with values in (-1, 1)
  (a column may repeat within a row; its entries add up), the diagonal entry = the row's sum of |values| + margin,
  so the matrix is strictly row diagonally dominant and non-singular; then a fraction `negative_rows` of the rows,
  picked at random, is negated whole, which gives negative diagonals and keeps the matrix non-singular.  The
  diagonal entry is stored last in its row.
"""
from __future__ import annotations

import numpy as np

from .spd import _csr, spmv64  # noqa: F401  (spmv64: host checks, as for spd)


def _convdiff(shape, wind):
    dims = len(shape)
    winds = np.broadcast_to(np.asarray(wind, np.float64), (dims,))
    if np.any(winds < 0):
        raise ValueError("wind must be >= 0 on every axis")
    n = int(np.prod(shape))
    idx = np.arange(n, dtype=np.int64).reshape(shape)
    rows = [idx.ravel()]
    cols = [idx.ravel()]
    vals = [np.full(n, 2.0 * dims + float(winds.sum()), np.float64)]
    for axis in range(dims):
        for step in (-1, 1):
            src = [slice(None)] * dims
            dst = [slice(None)] * dims
            if step < 0:                                # neighbour at index - 1: upstream for a wind >= 0
                src[axis], dst[axis] = slice(1, None), slice(None, -1)
            else:
                src[axis], dst[axis] = slice(None, -1), slice(1, None)
            r = idx[tuple(src)].ravel()
            rows.append(r)
            cols.append(idx[tuple(dst)].ravel())
            vals.append(np.full(r.size, -1.0 - (winds[axis] if step < 0 else 0.0), np.float64))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    return _csr(n, rows[order], cols[order], vals[order])


def convdiff2d(m, wind=1.0):
    return _convdiff((m, m), wind)


def convdiff3d(m, wind=1.0):
    return _convdiff((m, m, m), wind)


def random_nonsym(n, k=7, seed=0, margin=1.0, negative_rows=0.0):
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n, dtype=np.int64), k)
    c = rng.integers(0, n, size=r.size, dtype=np.int64)
    c = np.where(c == r, (c + 1) % n, c)                   # off-diagonal only
    v = rng.uniform(-1.0, 1.0, size=r.size).astype(np.float32)
    d = (np.bincount(r, weights=np.abs(v).astype(np.float64), minlength=n) + margin).astype(np.float32)
    if negative_rows > 0.0:
        flip = rng.random(n) < negative_rows
        v = np.where(flip[r], -v, v)
        d = np.where(flip, -d, d)
    diag = np.arange(n, dtype=np.int64)
    rows = np.concatenate([r, diag])
    cols = np.concatenate([c, diag])
    vals = np.concatenate([v, d])
    order = np.argsort(rows, kind="stable")
    return _csr(n, rows[order], cols[order], vals[order])
