"""Graphs at the structure limits of the tile builder (csrc/tiles.hip) and the per-tile error measure of the tests that run
every tile kernel on them (tests/test_gpu_plan_limits.py; tests/test_host_plan_limits.py checks both on the CPU).

The limits: <= 512 distinct halo nodes per tile (HALO_CAP; 256 + 512 = 768 LDS rows), <= 255 pair-merged slots per node
(``slice_deg`` is a uint8), <= 4 096 halo candidates per tile (CAND_CAP, both edge directions counted as ``k_halo`` does),
<= 4 096 nodes per sort cell (SORT_CAP), and on mixed plans <= 682 tile + halo rows (MIXED_ROW_CAP: the Neumann tiles' JVP
keeps 240 bytes per LDS row).  Each case comes at its limit (the plan must tile) and one past it (it must fall back).

The graphs carry no ``pos`` (except the sort-cell cases): the plan then keeps the given numbering and its tiles are
consecutive chunks of ``tile_target`` nodes, which fixes exactly which nodes share a tile and what each tile's halo is.
Tile 0 (nodes 0..255) is the limit tile; it holds no Dirichlet node, and on mixed graphs every fifth node of it is a
Neumann node (node 0, the deep-slot node, among them)."""
from dataclasses import dataclass, field

import numpy as np
import torch

from plan_ref import merge_slots, plan_reference

TILE = 256
HALO_CAP, SLOT_CAP, CAND_CAP, SORT_CAP = 512, 255, 4096, 4096
MIXED_ROW_CAP = 160 * 1024 // (60 * 4)          # 682
MIRROR = np.array([-1.0, -1.0, 1.0], dtype=np.float32)


@dataclass
class Case:
    name: str
    mixed: bool
    mesh: object                    # MeshData (CPU)
    tile_target: int                # MeshPlan tile_target (0: library default, 256 nodes)
    tiled: bool                     # expected outcome of the tile builder
    halo_cnt: dict = field(default_factory=dict)     # tile -> distinct halo nodes
    slice_deg: dict = field(default_factory=dict)    # slice -> slot rows
    cand: dict = field(default_factory=dict)         # tile -> halo candidates
    max_rows: int = None            # max over tiles of tile + halo rows (None: not fixed by the construction)
    slot_node: int = None           # the node with the deepest slot walk (caller's numbering)


class _Edges:
    """Directed edges with their attrs; mutual() adds the exact mirror pair the tile builder merges into one slot."""

    def __init__(self, rng):
        self.rng, self.src, self.dst, self.attr = rng, [], [], []

    def one(self, u, v, a=None):
        self.src.append(u)
        self.dst.append(v)
        self.attr.append(self.rng.standard_normal(3).astype(np.float32) if a is None else a)

    def mutual(self, u, v, mirror=True):
        a = self.rng.standard_normal(3).astype(np.float32)
        self.one(u, v, a)
        self.one(v, u, a * MIRROR if mirror else None)

    def chain(self, nodes):
        for u, v in zip(nodes[:-1], nodes[1:]):
            self.mutual(int(u), int(v))


def _mesh(N, E, mixed, rng, protect, pos=None):
    """MeshData: the edges of E (in shuffled order) plus one self loop per node, random x, a_ij, prb_data; tags with no
    Dirichlet node in ``protect`` and, on mixed graphs, every fifth protected node a Neumann node; unit normals."""
    from conftest import pkg
    ei = np.concatenate([np.stack([np.asarray(E.src), np.asarray(E.dst)]), np.stack([np.arange(N)] * 2)], axis=1)
    ea = np.concatenate([np.stack(E.attr), np.zeros((N, 3), np.float32)], axis=0)
    order = rng.permutation(ei.shape[1])
    ei, ea = ei[:, order], ea[order]
    prot = np.zeros(N, bool)
    prot[list(protect)] = True
    kind = np.where(rng.random(N) < 0.1, 1, 0)
    if mixed:
        kind = np.where(rng.random(N) < 0.1, 2, kind)
        kind[prot] = 0
        kind[np.flatnonzero(prot)[::5]] = 2
        tags = np.eye(3, dtype=np.float32)[kind]
    else:
        kind[prot] = 0
        tags = kind.reshape(-1, 1).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    m = pkg("data").MeshData(x=t(rng.standard_normal((N, 1)).astype(np.float32)), edge_index=t(ei.astype(np.int64)),
                             edge_attr=t(ea), a_ij=t(rng.standard_normal((ei.shape[1], 1)).astype(np.float32)),
                             y=t(rng.standard_normal((N, 1)).astype(np.float32)), sol=torch.zeros(N, 1),
                             prb_data=t(rng.standard_normal((N, 3 if mixed else 2)).astype(np.float32)), tags=t(tags),
                             pos=None if pos is None else t(pos.astype(np.float32)))
    if mixed:
        nv = rng.standard_normal((N, 2)).astype(np.float32)
        m.unit_normal_vector = t(nv / np.linalg.norm(nv, axis=1, keepdims=True))
    return m


def _chains(E, N, skip=()):
    """A mutual chain through the nodes of every 256-node tile (inside the tile only), leaving out the nodes in ``skip``."""
    for t0 in range(0, N, TILE):
        E.chain([i for i in range(t0, min(t0 + TILE, N)) if i not in skip])


def _halo_graph(h, mixed, rng, hub=False):
    """Tile 0 with exactly h halo nodes 256..256+h-1: halo node 256 + k is joined by a mirror pair to tile node k % 256.
    hub: node 0 is also joined to tile nodes 1..253, so it has 253 + 2 = 255 merged slots (h > 256)."""
    N = TILE + h
    E = _Edges(rng)
    for k in range(h):
        E.mutual(k % TILE, TILE + k)
    if hub:
        for v in range(1, 254):
            E.mutual(0, v)
    _chains(E, N, skip={0} if hub else ())
    return _mesh(N, E, mixed, rng, range(TILE)), N


def build(name, mixed, seed=0):
    """The case ``name`` in the family (mixed or dirichlet); see CASE_NAMES."""
    rng = np.random.default_rng(1000 + seed + (7 if mixed else 0) + sum(map(ord, name)))
    rows_cap = MIXED_ROW_CAP if mixed else TILE + HALO_CAP
    if name in ("halo512", "halo513", "jvp682", "jvp683"):
        h = {"halo512": 512, "halo513": 513, "jvp682": MIXED_ROW_CAP - TILE, "jvp683": MIXED_ROW_CAP - TILE + 1}[name]
        m, N = _halo_graph(h, mixed, rng)
        ok = h <= HALO_CAP and TILE + h <= rows_cap
        return Case(name, mixed, m, 0, ok, halo_cnt={0: h}, max_rows=TILE + h)
    if name == "halo_passes":
        # tiles 0..5 with halos of 0, 1, 255, 256, 257 and the largest the family tiles: 1, 2 and 3 LDS staging passes of
        # 256 rows (the third starts at row 512), and an empty halo; the halo nodes form the tiles after them
        halos = [0, 1, 255, 256, 257, rows_cap - TILE - (0 if mixed else 1)]
        n_src = len(halos) * TILE
        N = n_src + sum(halos)
        N += (-N) % TILE
        E = _Edges(rng)
        p = n_src
        for t, h in enumerate(halos):
            for k in range(h):
                E.mutual(t * TILE + k % TILE, p + k)
            p += h
        _chains(E, N)
        return Case(name, mixed, _mesh(N, E, mixed, rng, range(n_src)), 0, True,
                    halo_cnt=dict(enumerate(halos)),
                    max_rows=TILE + max(halos))
    if name in ("slots255", "slots256"):
        n = int(name[5:])
        N = 2 * TILE
        E = _Edges(rng)
        for v in range(1, n + 1):
            E.mutual(0, v)
        E.chain(list(range(1, N)))
        return Case(name, mixed, _mesh(N, E, mixed, rng, range(TILE)), 0, n <= SLOT_CAP, slice_deg={0: n}, slot_node=0)
    if name == "slots255_split":
        # node 0's 255 slots, none merged: 73 in-only (u -> 0), 60 out-only (0 -> u), 60 mutual pairs whose attrs are not
        # mirrors (an IN-only and an OUT-only slot each) and one in-edge given twice (two IN-only slots)
        N = 2 * TILE
        nb = rng.choice(np.arange(1, 400), size=73 + 60 + 60 + 1, replace=False)
        E = _Edges(rng)
        for u in nb[:73]:
            E.one(int(u), 0)
        for u in nb[73:133]:
            E.one(0, int(u))
        for u in nb[133:193]:
            E.mutual(0, int(u), mirror=False)
        a = rng.standard_normal(3).astype(np.float32)
        E.one(int(nb[193]), 0, a)
        E.one(int(nb[193]), 0, a)
        E.chain(list(range(1, N)))
        return Case(name, mixed, _mesh(N, E, mixed, rng, range(TILE)), 0, True, slice_deg={0: 255}, slot_node=0)
    if name == "both_limits":
        # the largest halo the family tiles and a 255-slot node in the same tile: the deepest slot walk over the most rows
        h = rows_cap - TILE
        m, N = _halo_graph(h, mixed, rng, hub=True)
        return Case(name, mixed, m, 0, True, halo_cnt={0: h}, slice_deg={0: 255}, max_rows=TILE + h, slot_node=0)
    if name in ("cand4096", "cand4097"):
        # 16 halo nodes 256..271, each tile node joined by mirror pairs to 8 of them: 256 * 8 * 2 = 4 096 candidates in
        # tile 0 and in tile 1 (the 16 nodes, 128 merged slots each); cand4097 adds the one-directional edge 0 -> 264
        N = TILE + 16
        E = _Edges(rng)
        for i in range(TILE):
            for k in range(8):
                E.mutual(i, TILE + (i + k) % 16)
        extra = name == "cand4097"
        if extra:
            E.one(0, TILE + 8)
        _chains(E, N)
        c = CAND_CAP + (1 if extra else 0)
        return Case(name, mixed, _mesh(N, E, mixed, rng, range(TILE)), 0, not extra, halo_cnt={0: 16, 1: TILE},
                    cand={0: c, 1: c}, max_rows=TILE + 16)
    if name.startswith("ragged"):
        # N = 3 * 256 + 1 with local random edges (some one-directional, some non-mirror) at tile sizes whose tiles end in
        # slices of 1..65 nodes
        tt = int(name[6:])
        N = 3 * TILE + 1
        E = _Edges(rng)
        for u in range(N):
            for d in rng.choice(np.arange(1, 12), size=4, replace=False):
                v = (u + int(d)) % N
                r = rng.random()
                if r < 0.8:
                    E.mutual(u, v)
                elif r < 0.9:
                    E.mutual(u, v, mirror=False)
                else:
                    E.one(u, v)
        return Case(name, mixed, _mesh(N, E, mixed, rng, range(TILE)), tt, True)
    if name in ("sort4096", "sort4097"):
        # with coordinates: n coincident points (one sort cell) and 300 points spread elsewhere, local edges by index
        n = int(name[4:])
        N = n + 300
        pos = np.zeros((N, 2))
        pos[n:] = 1.0 + rng.random((300, 2))
        E = _Edges(rng)
        for u in range(N - 3):
            E.mutual(u, u + 1)
            E.mutual(u, u + 3)
        return Case(name, mixed, _mesh(N, E, mixed, rng, range(TILE), pos=pos), 0, n <= SORT_CAP)
    raise KeyError(name)


CASE_NAMES = ["halo512", "halo513", "halo_passes", "jvp682", "jvp683", "slots255", "slots256", "slots255_split",
              "both_limits", "cand4096", "cand4097", "ragged32", "ragged63", "ragged65", "ragged100", "sort4096", "sort4097"]


# ------------------------------------------------------------------------------------------------ structure of a given tiling
def chunk_tiles(N, tile_target=0):
    """tile_ptr of a plan without coordinates: consecutive chunks of tile_target (default 256) nodes."""
    tt = TILE if tile_target <= 0 or tile_target > TILE else tile_target
    return np.array(list(range(0, N, tt)) + [N], dtype=np.int64)


def limits_of(edge_index, N, edge_attr, perm=None, tile_ptr=None):
    """What the tile builder measures against its limits for the tiling (perm[new] = old, tile_ptr): per tile the distinct
    halo nodes, the halo candidates (out-of-tile neighbours over the in- and the out-list) and the rows; per 64-lane slice
    the slot count (not clipped at 255).  Defaults: identity perm, 256-node chunks."""
    ref = plan_reference(edge_index, N)
    perm = np.arange(N) if perm is None else np.asarray(perm, dtype=np.int64)
    tile_ptr = chunk_tiles(N) if tile_ptr is None else np.asarray(tile_ptr, dtype=np.int64)
    inv = np.empty(N, dtype=np.int64)
    inv[perm] = np.arange(N)
    ea_bits = np.ascontiguousarray(np.asarray(edge_attr, dtype=np.float32)).view(np.uint32)
    halo, cand, slots = [], [], []
    for t in range(len(tile_ptr) - 1):
        t0, t1 = int(tile_ptr[t]), int(tile_ptr[t + 1])
        outside, nslot = [], []
        for new in range(t0, t1):
            old = perm[new]
            si = slice(ref["csc_ptr"][old], ref["csc_ptr"][old + 1])
            so = slice(ref["csr_ptr"][old], ref["csr_ptr"][old + 1])
            nb = inv[np.concatenate([ref["csc_nbr"][si], ref["csr_nbr"][so]]).astype(np.int64)]
            outside.append(nb[(nb < t0) | (nb >= t1)])
            nslot.append(len(merge_slots(ref["csc_nbr"][si], ref["csc_eid"][si], ref["csr_nbr"][so], ref["csr_eid"][so], ea_bits)))
        o = np.concatenate(outside) if outside else np.zeros(0, np.int64)
        halo.append(len(np.unique(o)))
        cand.append(len(o))
        slots += [max(nslot[w:w + 64]) for w in range(0, t1 - t0, 64)]
    halo = np.array(halo)
    return {"halo_cnt": halo, "cand": np.array(cand), "slice_deg": np.array(slots), "rows": np.diff(tile_ptr) + halo}


def should_tile(lim, mixed):
    """The builder's decision from limits_of (the sort-cell limit aside)."""
    return bool(lim["halo_cnt"].max() <= HALO_CAP and lim["cand"].max() <= CAND_CAP and lim["slice_deg"].max() <= SLOT_CAP
                and (not mixed or lim["rows"].max() <= MIXED_ROW_CAP))


# ------------------------------------------------------------------------------------------------ per-tile error measure
def tile_errors(got, want64, perm, tile_ptr):
    """e_t = |got - want|_t / max(|want|_t, 1e-3 |want| sqrt(n_t / N)) over the rows of every tile t (caller's numbering:
    tile t holds the nodes perm[tile_ptr[t]:tile_ptr[t + 1]])."""
    g = torch.as_tensor(got).detach().cpu().double().reshape(len(perm), -1)
    w = torch.as_tensor(want64).detach().cpu().double().reshape(len(perm), -1)
    N, wn = len(perm), float(w.norm())
    out = np.empty(len(tile_ptr) - 1)
    for t in range(len(tile_ptr) - 1):
        idx = torch.from_numpy(np.asarray(perm[tile_ptr[t]:tile_ptr[t + 1]], dtype=np.int64))
        n_t = len(idx)
        den = max(float(w[idx].norm()), 1e-3 * wn * np.sqrt(n_t / N))
        out[t] = float((g[idx] - w[idx]).norm()) / den if den > 0 else float((g[idx] - w[idx]).norm())
    return out


def check_tiles(got, want64, want32, perm, tile_ptr, tau, what, named=()):
    """Every tile: e_t <= max(16 e32_t, tau), e32_t the same measure of the float32 oracle (the 16x convention of
    tests/recurrences.py).  ``named``: tiles that must be in the measure (the limit tiles).  Returns (worst e_t, its e32_t)."""
    e = tile_errors(got, want64, perm, tile_ptr)
    e32 = tile_errors(want32, want64, perm, tile_ptr)
    bound = np.maximum(16 * e32, tau)
    for t in named:
        assert 0 <= t < len(e), (what, "named tile", t, len(e))
    bad = np.flatnonzero(~(e <= bound))
    assert bad.size == 0, (what, {int(t): (float(e[t]), float(bound[t])) for t in bad[:8]})
    k = int(np.argmax(e))
    return float(e[k]), float(e32[k])


def check_params(got, want64, want32, tau, what):
    """Parameter gradients tensor by tensor: e_k = |got_k - want_k| / max(|want_k|, 1e-4 scale) (scale: the largest |want_k|)
    <= max(tau, 16 e32_k), e32_k the same measure of the float32 oracle.  Returns (worst e_k, its e32_k)."""
    scale = max(float(t.double().norm()) for t in want64.values())
    err = lambda a, b: float((a.detach().cpu().double() - b.double()).norm()) / max(float(b.double().norm()), 1e-4 * scale)
    bad, worst = {}, (0.0, 0.0)
    for k, w in want64.items():
        e, e32 = err(got[k], w), err(want32[k], w)
        if not e <= max(tau, 16 * e32):
            bad[k] = (e, e32)
        worst = max(worst, (e, e32))
    assert not bad, (what, bad)
    return worst
