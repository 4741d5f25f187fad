"""Block CSR by numpy, the reference of tests/test_gpu_tangent_bsr.py: the CSR arrays of a matrix whose d x d blocks are
structurally dense (every node pair holds all its entries, nlps_gpu_tangent_csr) rearranged into block rows, every
block or the blocks with block column >= block row; and the dense matrix of such arrays, the upper form completed by
symmetry.  Nothing here adds or rounds: values move, bit for bit."""
import numpy as np


def bsr_from_csr(row_ptr, cols, vals, d, upper=False):
    """(brow_ptr[nb + 1], bcols[nblocks], bvals[nblocks, d, d]) of the CSR matrix (row_ptr, cols, vals) with nb * d rows;
    bvals[q][i][j] is the entry (A d + i, B d + j) of block q = (A, B).  upper: only the blocks with B >= A, the diagonal
    block whole.  The CSR columns must ascend inside every row and come in whole blocks (asserted)."""
    row_ptr, cols, vals = np.asarray(row_ptr), np.asarray(cols), np.asarray(vals)
    nrows = row_ptr.size - 1
    assert nrows % d == 0 and row_ptr[0] == 0 and row_ptr[-1] == cols.size == vals.size
    nb = nrows // d
    brow_ptr = np.zeros(nb + 1, dtype=np.int32)
    bcols, bvals = [], []
    for A in range(nb):
        lo, hi = row_ptr[A * d], row_ptr[A * d + 1]
        first = cols[lo:hi]
        assert first.size % d == 0
        blk = first.reshape(-1, d)
        assert np.array_equal(blk, blk[:, :1] + np.arange(d)) and not (blk[:, 0] % d).any(), "columns come in whole blocks"
        B = blk[:, 0] // d
        assert (np.diff(B) > 0).all(), "columns ascend"
        rows = np.empty((B.size, d, d))
        for i in range(d):
            a, b = row_ptr[A * d + i], row_ptr[A * d + i + 1]
            assert np.array_equal(cols[a:b], first), "the d rows of a node hold the same columns"
            rows[:, i, :] = vals[a:b].reshape(-1, d)
        keep = B >= A if upper else np.ones(B.size, dtype=bool)
        bcols.append(B[keep])
        bvals.append(rows[keep])
        brow_ptr[A + 1] = brow_ptr[A] + int(keep.sum())
    if nb == 0 or brow_ptr[-1] == 0:
        return brow_ptr, np.zeros(0, dtype=np.int32), np.zeros((0, d, d))
    return brow_ptr, np.concatenate(bcols).astype(np.int32), np.concatenate(bvals)


def csr_of_dense(K, d):
    """CSR arrays of the dense K that keep every entry of a d x d block with a non-zero in it"""
    n = K.shape[0]
    nb = n // d
    present = np.abs(K.reshape(nb, d, nb, d)).max(axis=(1, 3)) > 0
    full = np.repeat(np.repeat(present, d, axis=0), d, axis=1)
    row_ptr = np.concatenate([[0], np.cumsum(full.sum(axis=1))]).astype(np.int32)
    rows, cols = np.nonzero(full)
    return row_ptr, cols.astype(np.int32), K[rows, cols]


def dense_of_bsr(brow_ptr, bcols, bvals, d, upper=False, col_major=False):
    """The dense matrix of block CSR arrays.  upper: the arrays hold the blocks B >= A of a symmetric matrix, and the
    blocks below the diagonal are the transposes of those above it (the diagonal blocks are stored whole and taken as
    they are).  col_major: bvals[q] holds the transposed block."""
    brow_ptr, bcols = np.asarray(brow_ptr), np.asarray(bcols)
    bvals = np.asarray(bvals).reshape(-1, d, d)
    nb = brow_ptr.size - 1
    K = np.zeros((nb * d, nb * d))
    for A in range(nb):
        for q in range(brow_ptr[A], brow_ptr[A + 1]):
            B = int(bcols[q])
            blk = bvals[q].T if col_major else bvals[q]
            K[A * d:(A + 1) * d, B * d:(B + 1) * d] = blk
            if upper:
                assert B >= A, "an upper form holds no block below the diagonal"
                if B > A:
                    K[B * d:(B + 1) * d, A * d:(A + 1) * d] = blk.T
    return K


def ascending(brow_ptr, bcols):
    """block columns strictly ascending inside every block row"""
    return all((np.diff(np.asarray(bcols[a:b], dtype=np.int64)) > 0).all() for a, b in zip(brow_ptr[:-1], brow_ptr[1:]))


def diagonal_blocks(brow_ptr, bcols):
    """block rows that hold their diagonal block"""
    return sum(int(A in bcols[a:b]) for A, (a, b) in enumerate(zip(brow_ptr[:-1], brow_ptr[1:])))
