"""Integer triangular systems whose fp32 solve is exact in ANY summation order, with a prover in Python ints.

make(seed, uplo, unit, widths) builds a square CSR matrix whose `uplo` triangle T has a prescribed level structure:
block t of `widths` holds widths[t] rows and every row of it takes entries from the block before it (and some from
earlier ones), so level(row) = t.  Entries are small non-zero integers; the diagonal is a power of two (NON_UNIT) or,
with unit, an arbitrary stored value the solve must ignore.  The other triangle holds junk the solve must skip.  The
solution x is drawn first (integers) and b = T x is computed in Python ints.

prove(case) returns True when, for every row, sum_j |a_ij x_j| over the triangle INCLUDING the diagonal term stays
below 2**24: then every partial sum of the row in any order (with or without fused multiply-adds) is an integer below
2**24 and hence exact, b_i and b_i - s are exact, and the division by a power of two is exact; by induction over the
levels the computed x equals the integer solution bit for bit.  cases() regenerates what the prover rejects: nothing
is skipped.
"""
import numpy as np

LIMIT = 1 << 24


class Case:
    def __init__(self, name, n, rp, ci, va, b, x, uplo, unit, widths):
        self.name, self.n, self.rp, self.ci, self.va = name, n, rp, ci, va
        self.b, self.x, self.uplo, self.unit, self.widths = b, x, uplo, unit, widths


def make(seed, uplo, unit, widths, max_len=90, x_mag=900, a_mag=60):
    rng = np.random.default_rng(seed)
    n = int(sum(widths))
    starts = np.concatenate([[0], np.cumsum(widths)])
    x = rng.integers(-x_mag, x_mag + 1, n)
    rows, cols, vals = [], [], []
    for t, width in enumerate(widths):
        for p in range(int(starts[t]), int(starts[t + 1])):
            entries = {}
            if t > 0:
                # row lengths from 1 to max_len, so that every lane count meets rows shorter and longer than it
                k = int(rng.choice([1, 2, 3, 5, 9, 17, 33, 65, max_len]))
                prev = rng.integers(starts[t - 1], starts[t], 1)
                any_earlier = rng.integers(0, starts[t], max(k - 1, 0))
                for c in np.concatenate([prev, any_earlier]).tolist():
                    entries[c] = int(rng.choice([-1, 1])) * int(rng.integers(1, a_mag + 1))
            # junk in the other triangle
            for c in rng.integers(p + 1, n, int(rng.integers(0, 4))).tolist() if p + 1 < n else []:
                entries[c] = int(rng.integers(-a_mag, a_mag + 1)) or 7
            entries[p] = 3 if unit else 1 << int(rng.integers(0, 5))
            keys = list(entries)
            rng.shuffle(keys)                      # storage order is not column order
            for c in keys:
                rows.append(p)
                cols.append(c)
                vals.append(entries[c])
    rows, cols, vals = np.array(rows), np.array(cols), np.array(vals)
    if uplo == 1:                                  # mirror: position p -> n - 1 - p turns the lower structure upper
        rows, cols, x = n - 1 - rows, n - 1 - cols, x[::-1].copy()
    order = np.argsort(rows, kind="stable")
    rows, cols, vals = rows[order], cols[order], vals[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    inside = (cols < rows) if uplo == 0 else (cols > rows)
    b = [0] * n
    for r, c, v, tri in zip(rows.tolist(), cols.tolist(), vals.tolist(), inside.tolist()):
        if tri:
            b[r] += v * int(x[c])
        elif r == c:
            b[r] += (1 if unit else v) * int(x[c])
    name = f"seed{seed}-{'upper' if uplo else 'lower'}-{'unit' if unit else 'pow2'}-{len(widths)}levels"
    return Case(name, n, rp.astype(np.int32), cols.astype(np.int32), vals.astype(np.float32),
                np.array(b, dtype=np.int64), x.astype(np.int64), uplo, unit, list(widths))


def prove(case):
    """Python ints only."""
    rp, ci, va = case.rp.tolist(), case.ci.tolist(), [int(v) for v in case.va.tolist()]
    x = [int(v) for v in case.x.tolist()]
    for i in range(case.n):
        total = 0
        diagonals = 0
        for j in range(rp[i], rp[i + 1]):
            c = ci[j]
            if c == i:
                diagonals += 1
                d = 1 if case.unit else va[j]
                if d <= 0 or d & (d - 1):
                    return False               # not a power of two
                total += abs(d * x[i])
            elif (c < i) if case.uplo == 0 else (c > i):
                total += abs(va[j] * x[c])
        if diagonals != 1 or total >= LIMIT or abs(int(case.b[i])) >= LIMIT:
            return False
    return True


def cases(specs):
    """specs: (seed, uplo, unit, widths).  Every spec yields a proven case: a rejected draw is regenerated with the
    next seed (at most 50 times, then the generator itself is wrong)."""
    out = []
    for seed, uplo, unit, widths in specs:
        for attempt in range(50):
            case = make(seed + 1000 * attempt, uplo, unit, widths)
            if prove(case):
                out.append(case)
                break
        else:
            raise AssertionError(f"no provable case for {(seed, uplo, unit, widths)}")
    return out
