"""spd.py — symmetric positive definite test and benchmark matrices for cg_solve, in numpy only.

Every function returns (n, row_ptrs int32, col_indices int32, values float32) of a square CSR matrix:
* poisson2d(m): the 5-point Laplacian on an m x m grid (diagonal 4, neighbours -1), n = m^2, columns sorted;
* poisson3d(m): the 7-point Laplacian on an m^3 grid (diagonal 6, neighbours -1), n = m^3, columns sorted;
* random_spd(n, k, seed): S + S^T + D with k random off-diagonal columns per row of S (values in (-1, 1)),
  D_ii = sum_j |S_ij| + sum_j |S_ji| + margin: symmetric, strictly diagonally dominant with a positive diagonal,
  hence SPD.  Columns are scattered; a row's entries are not sorted and may repeat a column (the stored entries
  of a column add up, as for every CSR kernel of the library).
"""
from __future__ import annotations

import numpy as np


def _grid_laplacian(shape):
    dims = len(shape)
    n = int(np.prod(shape))
    idx = np.arange(n, dtype=np.int64).reshape(shape)
    rows = [idx.ravel()]
    cols = [idx.ravel()]
    vals = [np.full(n, 2.0 * dims, np.float32)]
    for axis in range(dims):
        for step in (-1, 1):
            src = [slice(None)] * dims
            dst = [slice(None)] * dims
            if step < 0:
                src[axis], dst[axis] = slice(1, None), slice(None, -1)
            else:
                src[axis], dst[axis] = slice(None, -1), slice(1, None)
            r = idx[tuple(src)].ravel()
            rows.append(r)
            cols.append(idx[tuple(dst)].ravel())
            vals.append(np.full(r.size, -1.0, np.float32))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    return _csr(n, rows[order], cols[order], vals[order])


def _csr(n, rows, cols, vals):
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return n, rp.astype(np.int32), cols.astype(np.int32), vals.astype(np.float32)


def poisson2d(m):
    return _grid_laplacian((m, m))


def poisson3d(m):
    return _grid_laplacian((m, m, m))


def random_spd(n, k=7, seed=0, margin=1.0):
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n, dtype=np.int64), k)
    c = rng.integers(0, n, size=r.size, dtype=np.int64)
    c = np.where(c == r, (c + 1) % n, c)                   # off-diagonal only
    v = rng.uniform(-1.0, 1.0, size=r.size).astype(np.float32)
    absv = np.abs(v).astype(np.float64)
    d = np.bincount(r, weights=absv, minlength=n) + np.bincount(c, weights=absv, minlength=n) + margin
    rows = np.concatenate([r, c, np.arange(n, dtype=np.int64)])
    cols = np.concatenate([c, r, np.arange(n, dtype=np.int64)])
    vals = np.concatenate([v, v, d.astype(np.float32)])
    order = np.argsort(rows, kind="stable")
    return _csr(n, rows[order], cols[order], vals[order])


def spmv64(rp, ci, va, x):
    """A x in fp64 (host checks: true residuals)."""
    rp = np.asarray(rp, np.int64)
    prod = np.asarray(va, np.float64) * np.asarray(x, np.float64)[ci]
    out = np.zeros(rp.size - 1, np.float64)
    nonempty = rp[1:] > rp[:-1]
    if prod.size and nonempty.any():
        out[nonempty] = np.add.reduceat(prod, rp[:-1][nonempty])
    return out
