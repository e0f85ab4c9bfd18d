"""Plain numpy float64 statement of the recurrences of csrc/poisson_cg.hip (Jacobi-preconditioned conjugate gradient on the lifted
system of the free rows), and the host-side pieces the tests of the device solve share."""
import numpy as np
import scipy.sparse as sp
import torch


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


def pcg_trace(A, y, dmask, tol, max_iter, x0=None):
    """(x, [|r_k| / |b|]) of the same recurrences: z = r / d, p = z + beta p, q = A p, alpha = r.z / p.q.  ``x0``: (N) start, its
    free rows are read (default zeros).  Like the device it stops at the first p.q <= 0 and returns the iterate before it."""
    Aff, b, F = lifted(A, y, dmask)
    d = Aff.diagonal()
    x = np.zeros_like(b) if x0 is None else np.asarray(x0, dtype=np.float64).reshape(-1)[F].copy()
    r = b - Aff @ x
    z = r / d
    p, rz, bn = np.zeros_like(b), r @ z, np.sqrt(b @ b)
    beta, trace = 0.0, [np.sqrt(r @ r) / bn]
    while trace[-1] > tol and len(trace) <= max_iter:
        p = z + beta * p
        q = Aff @ p
        if not p @ q > 0.0:
            break
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


# ------------------------------------------------------------------------------------------------ matrices that are not meshes
def mesh_of_entries(N, r, c, a, y, dmask, rng, dtype=np.float64):
    """MeshData (dirichlet family, no coordinates) whose matrix is the entry list (r, c, a) exactly as given -- the order of the
    entries is their edge id, an entry given twice stays two entries.  The fields the network reads are random filler."""
    from conftest import pkg
    E = len(r)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    return pkg("data").MeshData(x=t(f32(N, 1)), edge_index=t(np.stack([r, c]).astype(np.int64)), edge_attr=t(f32(E, 3)),
                                a_ij=t(np.asarray(a, dtype=dtype).reshape(E, 1)), y=t(np.asarray(y, dtype=dtype).reshape(N, 1)),
                                sol=torch.zeros(N, 1), prb_data=t(f32(N, 2)),
                                tags=t(np.asarray(dmask, dtype=np.float32).reshape(N, 1)), pos=None)


def spd_entries(N, pairs, rng, slack=0.25):
    """(r, c, a) in shuffled order: per undirected pair a weight w in U(0.5, 1.5) and a_uv = a_vu = -w; one self loop per node,
    a_uu = (1 + slack) sum of the node's w, or 1 for a node without pairs.  Strictly diagonally dominant, so symmetric positive
    definite, and so is every principal submatrix."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    pairs = np.unique(np.sort(pairs[pairs[:, 0] != pairs[:, 1]], axis=1), axis=0)
    u, v = pairs[:, 0], pairs[:, 1]
    w = rng.uniform(0.5, 1.5, len(pairs))
    s = np.zeros(N)
    np.add.at(s, u, w)
    np.add.at(s, v, w)
    diag = np.where(s > 0, (1.0 + slack) * s, 1.0)
    r, c, a = np.concatenate([u, v, np.arange(N)]), np.concatenate([v, u, np.arange(N)]), np.concatenate([-w, -w, diag])
    order = rng.permutation(len(r))
    return r[order], c[order], a[order]


def spd_problem(N, pairs, dmask, rng, slack=0.25, dtype=np.float64):
    """(MeshData, A csr float64) of spd_entries with a random right-hand side.  Dirichlet rows keep their values: the Dirichlet
    rows of A are NOT identity rows, so the truth is lifted_direct, not direct."""
    r, c, a = spd_entries(N, pairs, rng, slack)
    mesh = mesh_of_entries(N, r, c, a, rng.standard_normal(N), dmask, rng, dtype)
    return mesh, system(mesh, np.float32 if dtype == np.float32 else np.float64)[0]


def lifted_direct(A, y, dmask):
    """spsolve(A_FF, b) on the free rows, y on the Dirichlet rows -- whatever the Dirichlet rows of A hold."""
    from scipy.sparse.linalg import spsolve
    Aff, b, F = lifted(A, y, dmask)
    out = np.array(y, dtype=np.float64)
    if len(F):
        out[F] = np.atleast_1d(spsolve(Aff.tocsc(), b))
    return out


def kappa_gershgorin(A, dmask):
    """(1 + rho) / (1 - rho), rho = max_i sum_{j != i} |a_ij| / a_ii over A_FF: every eigenvalue of D^-1 A_FF lies within rho of 1
    (Gershgorin), and D^-1/2 A_FF D^-1/2 is similar to it, so this bounds cond(D^-1/2 A_FF D^-1/2) without an eigensolver.  At most
    9 for spd_entries at slack 0.25 (rho <= 1 / 1.25)."""
    Aff = lifted(A, np.zeros(A.shape[0]), dmask)[0]
    d = Aff.diagonal()
    off = np.asarray(abs(Aff).sum(axis=1)).reshape(-1) - np.abs(d)
    rho = float((off / d).max())
    assert (d > 0).all() and rho < 1.0, rho
    return (1.0 + rho) / (1.0 - rho)


def summed_entries(r, c, a):
    """{(i, j): sum of the entries given for the position}, each position summed in edge-id order as the device sums a run."""
    r, c, a = np.asarray(r, np.int64), np.asarray(c, np.int64), np.asarray(a, np.float64)
    out = {}
    for i, j, v in zip(r.tolist(), c.tolist(), a.tolist()):
        out[(i, j)] = out[(i, j)] + v if (i, j) in out else v
    return out


def symmetry_evidence(r, c, a, dmask):
    """What create judges a matrix by, on SUMMED entries over the free-free part: (sym_defect = max |A_ij - A_ji| over the
    off-diagonal positions that have a transposed position, max |A_ij| the diagonal included, whether a position has none)."""
    S = summed_entries(r, c, a)
    defect, amax, missing = 0.0, 0.0, False
    for (i, j), v in S.items():
        if dmask[i] or dmask[j]:
            continue
        amax = max(amax, abs(v))
        if i == j:
            continue
        if (j, i) in S:
            defect = max(defect, abs(v - S[(j, i)]))
        else:
            missing = True
    return defect, amax, missing


# ------------------------------------------------------------------------------------------------ the structure cases
HUB_DIRICHLET = tuple(range(64, 128)) + (303, 311, 319)
LONELY_DIRICHLET = (11, 12, 20, 40, 129) + tuple(range(64, 127))
STRUCTURE_CASES = ("hub321", "hub321_f32", "lonely", "band65536", "band65537")


def hub_pairs(N=321):
    """Node 0 joined to every other node, and a chain through 1..N-1."""
    return [(0, i) for i in range(1, N)] + [(i, i + 1) for i in range(1, N - 1)]


def _mask(N, rows):
    d = np.zeros(N, dtype=bool)
    d[list(rows)] = True
    return d


def lonely_pairs():
    """Every free row of ``lonely`` is alone or one of a pair (LONELY_DIRICHLET: the Dirichlet rows):
    5..9 and 63 have no entry but their diagonal; 0..4, 10, 127 and 128 have Dirichlet neighbours only (one to three of them);
    13..62 without 20 and 40 are 24 free pairs with no other neighbour; a chain runs through the Dirichlet rows 64..126.
    Slice 1 (rows 64..127) has the one free row 127 in lane 63, slice 2 (rows 128, 129) the one free row 128 in lane 0.
    Why pairs and not a chain: a 1 x 1 row is an eigenvector of D^-1 A_FF with eigenvalue 1, and conjugate gradients stopped at
    tol = 1e-12 leave it an error of that order (the numpy recurrences: 100 .. 450 ulp with a chain through the other free rows).
    A pair without other neighbours has a_uu = a_vv = 1.25 w, eigenvalues 0.2 and 1.8, so D^-1 A_FF has three distinct eigenvalues,
    the iteration ends in three steps at rounding level, and x_i = (y_i - sum a_ij y_j) / a_ii holds to a few ulp (numpy: 1.4),
    while kappa = 9 keeps the error gate off the float64 floor that a diagonal A_FF would put it on."""
    ch = [i for i in range(13, 63) if i not in (20, 40)]
    return ([(10, 11), (10, 12), (127, 126), (127, 64), (128, 129), (0, 11), (1, 12), (2, 20), (3, 40), (4, 11), (4, 12), (4, 20)]
            + [(i, i + 1) for i in range(64, 126)] + [(ch[k], ch[k + 1]) for k in range(0, len(ch), 2)])


def band_pairs(N, rng, reach=11, per_node=4):
    """Local random pairs: every node u is joined to ``per_node`` of the nodes u + 1 .. u + reach (those below N)."""
    u = np.repeat(np.arange(N), per_node)
    d = (np.argsort(rng.random((N, reach)), axis=1)[:, :per_node] + 1).reshape(-1)   # per_node distinct offsets per node
    keep = u + d < N
    return np.stack([u[keep], (u + d)[keep]], axis=1)


_cases = {}


def structure_case(name):
    """(MeshData on the host, A, y, dirichlet mask, lifted_direct solution, kappa_gershgorin) of a case of STRUCTURE_CASES --
    computed once, shared, never modified."""
    if name in _cases:
        return _cases[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    dtype = np.float32 if name.endswith("_f32") else np.float64
    if name.startswith("hub321"):
        mesh, _ = spd_problem(321, hub_pairs(), _mask(321, HUB_DIRICHLET), rng, dtype=dtype)
    elif name == "lonely":
        mesh, _ = spd_problem(130, lonely_pairs(), _mask(130, LONELY_DIRICHLET), rng)
        # y > 0 with a_ij < 0: b_i = y_i + sum w_ij y_j has no cancellation, so a 1 x 1 row's x_i is a few roundings from exact
        mesh.y = torch.from_numpy(rng.uniform(0.5, 1.5, (130, 1)))
    elif name.startswith("band"):
        N = int(name[4:])
        mesh, _ = spd_problem(N, band_pairs(N, rng), rng.random(N) < 0.1, rng)
    else:
        raise KeyError(name)
    A, y, dmask = system(mesh, dtype)
    _cases[name] = (mesh, A, y, dmask, lifted_direct(A, y, dmask), kappa_gershgorin(A, dmask))
    return _cases[name]


def one_by_one_rows(A, dmask):
    """The free rows whose off-diagonal columns are all Dirichlet columns (1 x 1 blocks of A_FF)."""
    return [i for i in np.flatnonzero(~dmask) if all(dmask[j] or j == i for j in A.indices[A.indptr[i]:A.indptr[i + 1]])]


def one_by_one_solution(A, y, i):
    """(y_i - sum_j a_ij y_j) / a_ii in exact rational arithmetic, rounded once."""
    from fractions import Fraction
    cols, vals = A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]]
    s = Fraction(float(y[i])) - sum(Fraction(float(v)) * Fraction(float(y[j])) for j, v in zip(cols, vals) if j != i)
    return float(s / Fraction(float(A[i, i])))


def gate(x, u, dmask, kappa, true_rel):
    """(|x - u|_F / |u|_F, kappa true_rel): for A_FF x = b, |x - u| / |u| <= cond(D^-1/2 A_FF D^-1/2) |b - A_FF x| / |b|."""
    F = ~dmask
    return float(np.linalg.norm((x - u)[F]) / np.linalg.norm(u[F])), kappa * true_rel


def true_rel_of(A, y, dmask, x):
    Aff, b, F = lifted(A, y, dmask)
    return float(np.linalg.norm(b - Aff @ x[F]) / np.linalg.norm(b))


# ------------------------------------------------------------------------------------------------ matrices create must judge
def in_pieces(r, c, a, rng):
    """The same matrix with every position given in pieces at shuffled edge ids.  Diagonal and upper (i < j) positions: two pieces,
    v/2 + v/2 for every other one, t v + (v - t v) with a random t otherwise.  Lower positions by turns: one piece (against
    v/2 + v/2: a symmetric matrix that an entry-by-entry comparison refuses), two pieces split and ordered differently from the
    transposed position's, three pieces.  A sum of pieces may differ from v in its last bit; symmetry_evidence says by how much."""
    R, C, V = [], [], []
    for n, (i, j, v) in enumerate(sorted(zip(r.tolist(), c.tolist(), a.tolist()))):
        t = float(rng.uniform(0.2, 0.8))
        if i <= j:
            parts = [v / 2, v / 2] if n % 2 == 0 else [t * v, v - t * v]
        else:
            parts = [[v], [v - t * v, t * v], [t * v / 2, v - t * v, t * v / 2]][n % 3]
        R += [i] * len(parts)
        C += [j] * len(parts)
        V += parts
    order = rng.permutation(len(R))
    return np.array(R)[order], np.array(C)[order], np.array(V)[order]


def entries_of(mesh):
    r, c = mesh.edge_index.numpy()
    return r.copy(), c.copy(), mesh.a_ij.numpy().reshape(-1).astype(np.float64)


def refused_matrices(r, c, a, dmask):
    """{name: ((r, c, a), what create's message must say)}: a valid matrix spoilt in one place each."""
    free = ~dmask
    ff = np.flatnonzero(free[r] & free[c] & (r != c))
    fd = np.flatnonzero(free[r] & dmask[c])
    dg = np.flatnonzero(free[r] & (r == c))
    drop = lambda k: (np.delete(r, k), np.delete(c, k), np.delete(a, k))
    put = lambda k, v: (r, c, np.concatenate([a[:k], [v], a[k + 1:]]))
    k = int(ff[5])
    return {"no transposed entry": (drop(k), "transposed"),
            "no diagonal entry": (drop(int(dg[7])), "diagonal"),
            "negative diagonal": (put(int(dg[9]), -a[dg[9]]), "diagonal"),
            "nan free-free": (put(int(ff[11]), np.nan), "not finite"),
            "inf in a dirichlet column": (put(int(fd[3]), np.inf), "not finite"),
            "v, v against v": ((np.append(r, r[k]), np.append(c, c[k]), np.append(a, a[k])), "symmetric")}


def garbage_in_dirichlet_rows(r, c, a, dmask, rng):
    """The same free rows; the Dirichlet rows lose their self loops and every other entry towards a free column, and what is left
    of them holds NaN, inf, -inf and random values by turns."""
    drow = dmask[r]
    k = np.flatnonzero(drow)
    gone = np.concatenate([k[r[k] == c[k]], k[(~dmask[c[k]])][::2]])
    a = a.copy()
    a[k] = np.where(np.arange(len(k)) % 4 == 3, rng.standard_normal(len(k)) * 1e300, np.resize([np.nan, np.inf, -np.inf, 0.0], len(k)))
    keep = np.setdiff1d(np.arange(len(r)), gone)
    return r[keep], c[keep], a[keep]
