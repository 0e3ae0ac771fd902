"""Device arrays as VIEWS into larger allocations, for tests/test_gpu_array_views.py.

Production callers hand the library interior pointers: a slice of a global CSR, a torch tensor's storage offset, a
vector inside a gathered buffer.  View puts a payload into one device allocation laid out as

    [8 poison | pad (poison) | payload | 8 poison]

with the payload starting `offset` elements (0..3) past a 16-byte boundary.  The poison is legal to read (a valid
column, an in-range row pointer, a finite value), so a stray read can never fault, but it cannot pass unnoticed in an
exact result (exact_data.VIEW_POISON, tests/test_exact_data.py); check_guards() shows a stray write bit for bit.

A plain module, not a conftest: imported by the GPU test only."""
import numpy as np

import exact_data as ed

GUARD = 8
SENTINEL = np.uint32(0x7FC0DEAD)          # test_gpu_spmv_multi.SENTINEL: the poison of output arrays


class View:
    """One caller-owned device allocation around `payload` (4-byte elements).  `poison` is a value of the payload's
    type, or an np.uint32 bit pattern (SENTINEL)."""

    def __init__(self, gpu, payload, offset, poison):
        payload = np.ascontiguousarray(payload)
        assert payload.dtype.itemsize == 4 and payload.ndim == 1 and 0 <= offset <= 3
        self.gpu, self.dtype, self.n, self.offset = gpu, payload.dtype, int(payload.size), offset
        bits = poison if isinstance(poison, np.uint32) else np.asarray(poison, self.dtype).reshape(1).view(np.uint32)[0]
        total = GUARD + 3 + self.n + GUARD
        self.buf = gpu.CudaBuffer(total, "uint32")
        base = self.buf.get()
        assert base % 4 == 0
        self.first = GUARD + (offset - base // 4 - GUARD) % 4
        self.ptr = base + 4 * self.first
        assert self.ptr % 16 == 4 * offset and GUARD <= self.first and self.first + self.n + GUARD <= total
        self.host = np.full(total, bits, np.uint32)
        self.host[self.first:self.first + self.n] = payload.view(np.uint32)
        self.buf.copyFromHost(self.host, total)

    def upload(self, payload):
        payload = np.ascontiguousarray(payload, self.dtype)
        assert payload.size == self.n
        self.host[self.first:self.first + self.n] = payload.view(np.uint32)
        self.buf.copyFromHost(self.host, self.host.size)

    def download(self):
        """The payload as the device holds it now."""
        return self.buf.copyToHost(self.host.size)[self.first:self.first + self.n].view(self.dtype).copy()

    def check_guards(self, what=""):
        """Everything outside the payload is what the constructor wrote, bit for bit."""
        now = self.buf.copyToHost(self.host.size)
        keep = np.ones(self.host.size, bool)
        keep[self.first:self.first + self.n] = False
        bad = np.flatnonzero(keep & (now != self.host))
        assert bad.size == 0, ("guard written", what, "offset", self.offset,
                               [(int(i) - self.first, hex(int(now[i]))) for i in bad[:8]])

    def release(self):
        self.buf.release()


class Views:
    """The views and the wrapped handles of one test case.  Leaving the block destroys the handles FIRST, then reads
    every guard (a wrapped handle owns nothing: the allocations must still be there), then frees the views."""

    def __init__(self, gpu):
        self.gpu, self.views, self.csr_handles, self.ell_handles = gpu, [], [], []

    def __enter__(self):
        return self

    def view(self, payload, offset, poison):
        v = View(self.gpu, payload, offset, poison)
        self.views.append(v)
        return v

    def x(self, x, offset):
        return self.view(np.asarray(x, np.float32), offset, np.float32(ed.VIEW_POISON))

    def out(self, count, offset):
        """An output vector: payload and guards all SENTINEL."""
        return self.view(np.full(count, SENTINEL, np.uint32).view(np.float32), offset, SENTINEL)

    def csr(self, rows, num_cols, rp, ci, va, offsets):
        """(handle, (rp view, cols view, vals view)) of csr_wrap_device over three views."""
        nnz = int(np.asarray(ci).size)
        v_rp = self.view(np.asarray(rp, np.int32), offsets[0], np.int32(nnz))
        v_ci = self.view(np.asarray(ci, np.int32), offsets[1], np.int32(num_cols - 1))
        v_va = self.view(np.asarray(va, np.float32), offsets[2], np.float32(ed.VIEW_POISON))
        A = self.gpu.csr_wrap_device(rows, num_cols, nnz, v_rp.ptr, v_ci.ptr, v_va.ptr)
        assert A is not None and not A.contents.owns_device_memory
        self.csr_handles.append(A)
        return A, (v_rp, v_ci, v_va)

    def ell(self, rows, num_cols, width, ecols, evals, offsets):
        """(handle, (cols view, vals view)) of ell_wrap_device over two slab views."""
        v_ci = self.view(np.asarray(ecols, np.int32), offsets[0], np.int32(num_cols - 1))
        v_va = self.view(np.asarray(evals, np.float32), offsets[1], np.float32(ed.VIEW_POISON))
        E = self.gpu.ell_wrap_device(rows, num_cols, width, v_ci.ptr, v_va.ptr)
        assert E is not None and not E.contents.owns_device_memory
        self.ell_handles.append(E)
        return E, (v_ci, v_va)

    def check_guards(self, what=""):
        for i, v in enumerate(self.views):
            v.check_guards((what, "view", i))

    def __exit__(self, kind, exc, tb):
        for A in self.csr_handles:
            self.gpu.csr_destroy(A)
        for E in self.ell_handles:
            self.gpu.ell_destroy(E)
        try:
            if kind is None:
                self.check_guards("after the handles were destroyed")
        finally:
            for v in self.views:
                v.release()
        return False
