"""Plain numpy float64 statement of the recurrences of csrc/poisson_cg.hip (Jacobi-preconditioned conjugate gradient on the lifted
system of the free rows), and the host-side pieces the tests of the device solve share."""
import numpy as np
import scipy.sparse as sp


def system(mesh, dtype=np.float64):
    """(A csr, y, dirichlet mask) of a MeshData in float64, from its tensors rounded to ``dtype`` first."""
    N = mesh.num_nodes
    r, c = mesh.edge_index.cpu().numpy()
    a = mesh.a_ij.cpu().numpy().reshape(-1).astype(dtype).astype(np.float64)
    y = mesh.y.cpu().numpy().reshape(-1).astype(dtype).astype(np.float64)
    tags = mesh.tags.cpu().numpy()
    dmask = (tags[:, 1] if tags.shape[1] == 3 else tags[:, 0]) == 1
    return sp.csr_matrix((a, (r, c)), shape=(N, N)), y, dmask


def lifted(A, y, dmask):
    """(A_FF, b = y_F - A_FD y_D, free index)."""
    F, Dn = np.flatnonzero(~dmask), np.flatnonzero(dmask)
    return A[F][:, F].tocsr(), y[F] - A[F][:, Dn] @ y[Dn], F


def pcg_trace(A, y, dmask, tol, max_iter):
    """(x, [|r_k| / |b|]) of the same recurrences: z = r / d, p = z + beta p, q = A p, alpha = r.z / p.q."""
    Aff, b, F = lifted(A, y, dmask)
    d = Aff.diagonal()
    x, r = np.zeros_like(b), b.copy()
    z = r / d
    p, rz, bn = np.zeros_like(b), r @ z, np.sqrt(b @ b)
    beta, trace = 0.0, [np.sqrt(r @ r) / bn]
    while trace[-1] > tol and len(trace) <= max_iter:
        p = z + beta * p
        q = Aff @ p
        alpha = rz / (p @ q)
        x, r = x + alpha * p, r - alpha * q
        z = r / d
        rz, rz_old = r @ z, rz
        beta = rz / rz_old
        trace.append(np.sqrt(r @ r) / bn)
    out = y.copy()
    out[F] = x
    return out, trace


def kappa_scaled(A, dmask, dense_limit=2000):
    """cond(D^-1/2 A_FF D^-1/2): numpy on the dense matrix up to ``dense_limit`` free rows, scipy's eigsh above."""
    Aff, _, _ = lifted(A, np.zeros(A.shape[0]), dmask)
    s = sp.diags(1.0 / np.sqrt(Aff.diagonal()))
    S = (s @ Aff @ s).tocsc()
    if S.shape[0] <= dense_limit:
        w = np.linalg.eigvalsh(S.toarray())
        return float(w[-1] / w[0])
    from scipy.sparse.linalg import eigsh
    hi = eigsh(S, k=1, which="LA", return_eigenvectors=False)[0]
    lo = eigsh(S, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0]
    return float(hi / lo)


def direct(A, y):
    from scipy.sparse.linalg import spsolve
    return spsolve(A.tocsc(), y)

