"""The numpy restatement of the parameter-gradient reduction geometry (tests/pgrad_ref.py) against the library, and the
regimes the at-scale gradient tests (tests/test_gpu_gradients_at_scale.py) claim to reach.  Host only:
psignn_mlp2_backward_workspace_floats(n) = 64 n + 512 nblk gives the library's block count without a GPU.  If pgrad_blocks
changes, the probes move with it or this test fails."""
import pytest

import pgrad_ref as pr
from conftest import pkg

MLP_LENGTHS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 262144, 262145, 1000519, 4194305]
N_270K, N_1M = 270901, 1000519          # make_hex_problem(300) / (577): 3 n (n + 1) + 1 nodes


def _library_blocks(n):
    ws = int(pkg("_native").lib().psignn_mlp2_backward_workspace_floats(n))
    assert (ws - 64 * n) % 512 == 0, (n, ws)
    return (ws - 64 * n) // 512


@pytest.mark.parametrize("n", sorted(set(MLP_LENGTHS + [N_270K, 2 * N_270K, N_1M, 2 * N_1M])))
def test_restated_block_count_matches_the_library(n):
    nblk, npw = pr.pgrad_blocks(n)
    assert _library_blocks(n) == nblk
    waves = pr.last_block_waves(n)
    assert sum(waves) == n - (nblk - 1) * pr.WAVES * npw and waves[0] > 0
    assert npw == 64 or n > 262144
    pos = pr.probes(n)
    assert all(len(p) > 0 and p.min() >= 0 and p.max() < n for p in pos.values())


# records -> (records per wave, the last block's waves): what each at-scale test relies on
REGIMES = {
    N_270K: (68, (68, 68, 68, 57)),          # npw > 64, every wave of the last block holds records, the fourth is ragged
    2 * N_270K: (136, (136, 136, 136, 114)),  # the same for the 2N records of the backward of the VJP
    N_1M: (248, (248, 248, 87, 0)),          # a ragged wave and an empty one
    2 * N_1M: (492, (492, 492, 492, 74)),
    1: (64, (1, 0, 0, 0)),
    262144: (64, (64, 64, 64, 64)),          # the last size with 64 records per wave
    262145: (68, (68, 68, 68, 5)),
}


@pytest.mark.parametrize("n", sorted(REGIMES))
def test_claimed_regimes(n):
    npw, waves = REGIMES[n]
    assert pr.pgrad_blocks(n)[1] == npw
    assert pr.last_block_waves(n) == waves
    if n == N_1M:
        assert 0 < waves[2] < npw and waves[3] == 0
    if n == N_270K or n == 2 * N_270K:
        assert npw > 64 and min(waves) > 0 and waves[3] < npw
    if n == 2 * N_270K:
        # the seam between the two record sets (N - 1 | N) falls inside a wave, and the seam probe holds it
        assert N_270K % npw != 0
        seam = pr.probes(n, seam=N_270K)["record-set seam"]
        assert seam.min() < N_270K - 1 and seam.max() > N_270K


def test_probe_positions():
    nblk, npw = pr.pgrad_blocks(N_1M)
    p = pr.probes(N_1M)
    assert list(p["first wave"]) == list(range(npw))
    assert p["last block"][0] == (nblk - 1) * 4 * npw and p["last block"][-1] == N_1M - 1
    mid = p["middle block boundary"]
    assert len(mid) == 4 * npw and (mid[0] + 2 * npw) % (4 * npw) == 0
    # the node of a record: order[p % N] (plan order on tiled paths, the caller's order on gather paths)
    order = list(reversed(range(10)))
    assert list(pr.nodes_at([0, 1, 10, 19], order, 10)) == [0, 8, 9]
