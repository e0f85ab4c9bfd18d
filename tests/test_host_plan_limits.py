"""CPU: the structure-limit graphs of tests/limit_graphs.py reach exactly the limits they are built for (so that the GPU test
tests/test_gpu_plan_limits.py cannot quietly turn into a test of small graphs), and the per-tile error checker it uses
rejects an f that is wrong only in the rows a limit tile reads from its third LDS staging pass or its 255th slot."""
import numpy as np
import pytest
import torch

import limit_graphs as lg
from conftest import load_weights, rel_l2
from oracle import psignn_oracle as orc
from plan_ref import tile_reference

NO_POS = [n for n in lg.CASE_NAMES if not n.startswith("sort")]


@pytest.mark.parametrize("mixed", [False, True], ids=["dirichlet", "mixed"])
@pytest.mark.parametrize("name", NO_POS)
def test_case_reaches_its_limit(name, mixed):
    case = lg.build(name, mixed)
    m = case.mesh
    N = m.num_nodes
    ei, ea = m.edge_index.numpy(), m.edge_attr.numpy()
    tile_ptr = lg.chunk_tiles(N, case.tile_target)
    lim = lg.limits_of(ei, N, ea, tile_ptr=tile_ptr)
    for t, h in case.halo_cnt.items():
        assert lim["halo_cnt"][t] == h, (t, lim["halo_cnt"][t], h)
    for s, d in case.slice_deg.items():
        assert lim["slice_deg"][s] == d, (s, lim["slice_deg"][s], d)
    for t, c in case.cand.items():
        assert lim["cand"][t] == c, (t, lim["cand"][t], c)
    if case.max_rows is not None:
        assert lim["rows"].max() == case.max_rows
    assert lg.should_tile(lim, mixed) == case.tiled
    # no limit is crossed but the one the case is about
    others = {"halo": lim["halo_cnt"].max() <= lg.HALO_CAP, "cand": lim["cand"].max() <= lg.CAND_CAP,
              "slots": lim["slice_deg"].max() <= lg.SLOT_CAP, "rows": not mixed or lim["rows"].max() <= lg.MIXED_ROW_CAP}
    crossed = {k for k, ok in others.items() if not ok}
    if "halo" in crossed:       # a mixed tile past 512 halo nodes is past 682 rows as well
        crossed.discard("rows")
    assert len(crossed) <= 1, crossed
    # the limit tile holds no Dirichlet node; mixed: Neumann nodes in it (the deep-slot node among them)
    tags = m.tags.numpy()
    dcol = tags[:, 1] if mixed else tags[:, 0]
    assert not dcol[:lg.TILE].any()
    if mixed:
        assert tags[:lg.TILE, 2].sum() >= 50 and (case.slot_node is None or tags[case.slot_node, 2] == 1)
    if case.tiled and name in ("halo512", "both_limits", "slots255_split", "cand4096", "ragged63"):
        # the numpy statement of the builder's output agrees (bit-exact reference of the GPU test)
        ref = tile_reference(ei, N, np.arange(N), tile_ptr, ea)
        assert np.array_equal(ref["halo_cnt"], lim["halo_cnt"])
        assert np.array_equal(ref["slice_deg"].astype(np.int64), lim["slice_deg"])
        if name == "slots255_split":   # node 0 (lane 0 of slice 0): 255 slots, none of them a merged pair
            kinds = ref["ell"][:255, 0, 0] >> 16
            assert len(kinds) == 255 and set(kinds.tolist()) == {1, 2}


@pytest.mark.parametrize("n", [4096, 4097])
def test_sort_case_fills_one_cell(n):
    case = lg.build(f"sort{n}", False)
    pos = case.mesh.pos.numpy()
    assert (np.abs(pos).sum(axis=1) == 0).sum() == n and pos[n:].min() >= 1.0
    assert case.tiled == (n <= lg.SORT_CAP)


def _f(sd, mesh, h, h0):
    with torch.no_grad():
        return orc.function_forward(sd, h.clone(), h0, mesh)


def _to64(sd, mesh):
    m64 = mesh.clone()
    for k, v in list(vars(mesh).items()):
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(m64, k, v.double())
    return {k: v.double() for k, v in sd.items()}, m64


def _drop_edges(mesh, bad):
    m = mesh.clone()
    keep = ~bad
    m.edge_index, m.edge_attr, m.a_ij = m.edge_index[:, keep], m.edge_attr[keep], m.a_ij[keep]
    return m


@pytest.mark.parametrize("corruption", ["halo_rows_from_512", "slot_255"])
def test_tile_checker_rejects_a_limit_defect(corruption):
    """f of the oracle in float64, then a copy whose limit-tile rows miss what a kernel would miss if its third staging pass
    (LDS rows >= 512) or its 255th slot row were lost.  The per-tile checker must name tile 0; the whole-vector rel-L2 is
    printed for comparison (it may well pass such a defect on a large graph)."""
    name = "halo512" if corruption == "halo_rows_from_512" else "slots255"
    case = lg.build(name, False)
    m = case.mesh
    N = m.num_nodes
    sd = load_weights("dirichlet")
    gen = torch.Generator().manual_seed(3)
    h0, h = 0.3 * torch.randn(N, 10, generator=gen), 0.3 * torch.randn(N, 10, generator=gen)
    sd64, m64 = _to64(sd, m)
    want64 = _f(sd64, m64, h.double(), h0.double())
    want32 = _f(sd, m, h, h0)
    ei = m.edge_index
    if corruption == "halo_rows_from_512":
        # tile 0's LDS row 256 + k holds halo node 256 + k: rows >= 512 are the nodes >= 512
        bad = ((ei[0] < lg.TILE) & (ei[1] >= 512)) | ((ei[1] < lg.TILE) & (ei[0] >= 512))
    else:
        # node 0's slots are its neighbours 1..255 in order: the 255th is node 255
        bad = ((ei[0] == 0) & (ei[1] == 255)) | ((ei[0] == 255) & (ei[1] == 0))
    assert int(bad.sum()) > 0
    bad_f = _f(sd64, _drop_edges(m64, bad), h.double(), h0.double())
    got = want64.clone()
    got[:lg.TILE] = bad_f[:lg.TILE]
    perm, tile_ptr = np.arange(N), lg.chunk_tiles(N)
    # the oracle itself passes; the corrupted copy fails in tile 0 and only there
    lg.check_tiles(want32, want64, want32, perm, tile_ptr, 2e-6, "oracle")
    with pytest.raises(AssertionError, match=r"\{0: "):
        lg.check_tiles(got, want64, want32, perm, tile_ptr, 2e-6, corruption)
    e = lg.tile_errors(got, want64, perm, tile_ptr)
    assert e[0] > 1e3 * 2e-6 and np.all(e[1:] == 0)
    print(corruption, "tile 0 error", e[0], "whole-vector rel-L2", rel_l2(got, want64))


def test_tile_error_floor():
    """A tile whose own rows are ~0 is measured against a share of the whole vector's norm, not against its own norm."""
    N = 512
    want = torch.ones(N, 10, dtype=torch.float64)
    want[:256] = 0.0
    got = want.clone()
    got[:256] = 1e-9
    e = lg.tile_errors(got, want, np.arange(N), lg.chunk_tiles(N))
    floor = 1e-3 * float(want.norm()) * np.sqrt(256 / N)
    assert np.isclose(e[0], float(torch.full((256, 10), 1e-9).norm()) / floor) and e[1] == 0
