"""The CSR block GpuCutSelectionMixin._separate_and_add_triangle builds on the host from the head of tri_separate, as a function:
its numpy code, copied once, for the triangle tests (test_triangles_cpu.py, test_gpu_tri_nodes.py) and tools/batch_points.py, which
compare the device's rows against it and time it.  A plain module: no fixtures, no GPU."""
import numpy as np


def numpy_rows(tri, n, ent):
    """the CSR block GpuCutSelectionMixin._separate_and_add_triangle builds from the head of tri_separate (its code)"""
    L = n * (n + 1) // 2
    e = np.asarray(ent, dtype=np.int64)
    c = (e & 3).astype(np.int64)
    tri64 = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    abd = tri64[e >> 2]
    a3, b3, d3 = abd[:, 0], abd[:, 1], abd[:, 2]
    ra, rb = n * a3 - a3 * (a3 + 1) // 2, n * b3 - b3 * (b3 + 1) // 2
    four = c < 3
    indptr = np.zeros(e.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.where(four, 4, 6), out=indptr[1:])
    pos = indptr[:-1]
    ind = np.empty(int(indptr[-1]), dtype=np.int64)
    val = np.empty(int(indptr[-1]), dtype=np.float64)
    ind[pos], ind[pos + 1], ind[pos + 2] = ra + b3, ra + d3, rb + d3
    p4, p6 = pos[four], pos[~four]
    ind[p4 + 3] = abd[four, c[four]] + L
    ind[p6 + 3], ind[p6 + 4], ind[p6 + 5] = a3[~four] + L, b3[~four] + L, d3[~four] + L
    v4 = np.array([[-1.0, -1.0, 1.0, 1.0], [-1.0, 1.0, -1.0, 1.0], [1.0, -1.0, -1.0, 1.0]])[c[four]]
    for j in range(4):
        val[p4 + j] = v4[:, j]
    for j, v in enumerate((1.0, 1.0, 1.0, -1.0, -1.0, -1.0)):
        val[p6 + j] = v
    return indptr, ind, val, np.where(four, 0.0, -1.0)
