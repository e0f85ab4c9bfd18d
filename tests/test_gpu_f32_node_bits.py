"""GPU: the float32 node block gives the bits of the recorded build.

The kernels that evaluate f_theta and its derivatives use fixed summation orders and no atomics, so a rearrangement of their
source that keeps every statement gives byte-identical outputs.  ``scripts/tile_bits.py`` prints a CRC-32 of the raw output bytes
of every entry point that runs one of them (tile and gather kernels, both families, one and two layers);
``tests/golden/f32_node_bits_parent.json`` holds its entries for ``make_hex_problem(13)`` -- 547 nodes, three tiles with a ragged
last tile; interior, Dirichlet and, in the mixed family, Neumann rows -- and this test recomputes them.

The golden is pinned to a gfx950 build of the commit before the duplicated helpers of these kernels got one definition in
``csrc/fgnn_common.h``.  A differing CRC is a changed statement (or a changed contraction of one by the
compiler), not noise.  After a deliberate change of the arithmetic, re-record with

    python scripts/tile_bits.py --out line.json

and store the ``hex13_dirichlet`` and ``hex13_mixed`` entries of that line.
"""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


def test_same_bits_as_the_recorded_build(dev):
    """Every hex13 entry of scripts/tile_bits.py, both families, equals the recorded one; the sets of keys are equal."""
    spec = importlib.util.spec_from_file_location("tile_bits", os.path.join(ROOT, "scripts", "tile_bits.py"))
    bits = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bits)
    with open(os.path.join(GOLDEN, "f32_node_bits_parent.json")) as f:
        want = json.load(f)
    assert set(want) == {"hex13_dirichlet", "hex13_mixed"}
    for mixed in (False, True):
        name = f"hex13_{'mixed' if mixed else 'dirichlet'}"
        got = bits.psignn(13, mixed, dev)
        assert set(got) == set(want[name]), (name, set(got) ^ set(want[name]))
        for key, value in want[name].items():
            assert got[key] == value, (name, key, got[key], value)
