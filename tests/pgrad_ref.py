"""The reduction geometry of the parameter-gradient kernels (csrc/fgnn_pgrad.hip), restated in numpy for the tests that aim
cotangent probes at its seams (tests/test_gpu_gradients_at_scale.py; tests/test_host_pgrad_geometry.py checks it against the
library).

k_pgrad_outer gives every wave of 64 lanes ``npw`` consecutive records and every block 4 waves; k_pgrad_reduce /
k_pgrad_reduce_acc add the per-block (or, for the wide tables, per-wave) partials.  Up to 262 144 records a wave owns 64;
past that ``npw`` grows (a multiple of 4) and the block count stays near 1 024, so the last block can hold a ragged wave and
waves with no record at all.  Record positions count in the order the records are written: plan order on the tiled paths,
the caller's order on the gather paths; the backward of the VJP writes two sets (node n at n and at N + n)."""
import numpy as np

WAVES = 4


def cdiv(a, b):
    return -(-a // b)


def pgrad_blocks(n):
    """(blocks, records per wave) of ``pgrad_blocks(n)``."""
    npw = max(64, cdiv(cdiv(n, 4096), 4) * 4)
    return cdiv(n, npw * WAVES), npw


def last_block_waves(n):
    """Records held by each of the last block's four waves."""
    nblk, npw = pgrad_blocks(n)
    b0 = (nblk - 1) * WAVES * npw
    return tuple(int(min(max(n - (b0 + k * npw), 0), npw)) for k in range(WAVES))


def probes(n, seam=None):
    """Record positions that sit at a reduction boundary, {name: positions}: the first wave; the whole last block (full,
    ragged and empty waves alike); the two waves on either side of the block boundary nearest the middle; and, with ``seam``
    (the first position of a second record set), the wave holding it and its two neighbours."""
    nblk, npw = pgrad_blocks(n)
    span = WAVES * npw
    out = {"first wave": np.arange(0, min(npw, n)),
           "last block": np.arange((nblk - 1) * span, n)}
    if nblk >= 2:
        b = (nblk // 2) * span
        out["middle block boundary"] = np.arange(b - 2 * npw, min(b + 2 * npw, n))
    if seam is not None:
        w = (seam // npw) * npw
        out["record-set seam"] = np.arange(max(w - npw, 0), min(w + 2 * npw, n))
    return out


def nodes_at(positions, order, n_nodes):
    """The nodes whose records sit at ``positions`` (record p belongs to node order[p % n_nodes]), sorted, unique."""
    return np.unique(np.asarray(order)[np.asarray(positions) % n_nodes])
