"""Shared helpers of tests/test_spgemm_host.py and tests/test_gpu_spgemm.py: CSR builders and the plain restatement of
the product's arithmetic (include/spmv/spgemm.h).  A plain module, not a conftest."""
import numpy as np


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def csr_from_rows(rows, num_rows=None):
    """(row_ptrs, cols, vals) from a list of rows, each a list of (col, value) in storage order."""
    num_rows = len(rows) if num_rows is None else num_rows
    rp = np.zeros(num_rows + 1, np.int32)
    ci, va = [], []
    for i, row in enumerate(rows):
        for c, v in row:
            ci.append(c)
            va.append(v)
        rp[i + 1] = len(ci)
    rp[len(rows) + 1:] = len(ci)
    return rp, np.asarray(ci, np.int32), np.asarray(va, np.float32)


def random_csr(rng, rows, cols, density, sort=True, duplicates=False, lo=-4.0, hi=4.0):
    """Random fp32 CSR; rows strictly ascending when sort, else shuffled, with repeated entries when duplicates."""
    out = []
    for _ in range(rows):
        count = int(rng.binomial(cols, density)) if cols else 0
        c = rng.choice(cols, size=count, replace=False) if count else np.empty(0, np.int64)
        if duplicates and count:
            c = np.concatenate([c, rng.choice(c, size=max(1, count // 3))])
        c = np.sort(c) if sort else rng.permutation(c)
        v = rng.uniform(lo, hi, size=c.size).astype(np.float32)
        out.append(list(zip(c.tolist(), v.tolist())))
    return csr_from_rows(out)


def product_loop(m, n, a, b):
    """The definition, as a plain double loop: per row, A's entries in storage order, each B row in storage order,
    acc = fl(acc + fl(a * b)); the touched columns ascending.  a, b = (row_ptrs, cols, vals)."""
    arp, aci, ava = a
    brp, bci, bva = b
    rp = np.zeros(m + 1, np.int32)
    ci, va = [], []
    with np.errstate(all="ignore"):
        for i in range(m):
            acc = {}
            for p in range(arp[i], arp[i + 1]):
                k, av = int(aci[p]), np.float32(ava[p])
                for q in range(brp[k], brp[k + 1]):
                    c = int(bci[q])
                    product = np.float32(av * np.float32(bva[q]))
                    acc[c] = np.float32(acc.get(c, np.float32(0.0)) + product)
            for c in sorted(acc):
                ci.append(c)
                va.append(acc[c])
            rp[i + 1] = len(ci)
    return rp, np.asarray(ci, np.int32), np.asarray(va, np.float32)


def host_product(spmv, m, k, n, a, b):
    """spgemm_cpu_csr of freshly built host matrices: (status, (row_ptrs, cols, vals))."""
    A = spmv.csr_from_arrays(m, k, *a)
    B = spmv.csr_from_arrays(k, n, *b)
    C = spmv.csr_create(0, 0, 0)
    status = spmv.spgemm_cpu_csr(C, A, B)
    got = spmv.csr_host_arrays(C) if status == 0 else None
    shape = (C.contents.num_rows, C.contents.num_cols, C.contents.nnz)
    for M in (A, B, C):
        spmv.csr_destroy(M)
    if status == 0:
        assert shape == (m, n, got[1].size)
    return status, got


def assert_same(got, want, what=""):
    """Row pointers, columns and value bits; NaNs compared by position (their payloads are not part of the rule)."""
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"row_ptrs {what}")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"cols {what}")
    g, w = np.asarray(got[2], np.float32), np.asarray(want[2], np.float32)
    np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f"NaN positions {what}")
    keep = ~np.isnan(w)
    np.testing.assert_array_equal(bits(g)[keep], bits(w)[keep], err_msg=f"value bits {what}")
