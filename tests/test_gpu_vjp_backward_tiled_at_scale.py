"""The tile form of the backward of the VJP (csrc/fgnn_tile_jr.hip) at 270 901 and 1 000 519 nodes against the CPU oracle in
float64, built on the mesh objects, probes, gates and SCALE report lines of test_gpu_gradients_at_scale.py.

The two record sets are written in PLAN order here (plan node n at n and N + n), so record position -> node goes through the
plan's ``perm``; the probes (first wave, last block, middle block boundary, the seam N - 1 | N between the sets) keep the
cotangent on the nodes behind those records and their neighbours and compare with the oracle on the two-hop sub-graph, which
is exact and cheap at any size.

* 270 901 nodes (541 802 records): dense comparison, tensor by tensor and tile by tile, then the probes.
* 1 000 519 nodes (2 001 038 records, npw = 492): the probes, and the dense comparison as well.  Its references are the
  float64 and (for the 16 e32 rule) the float32 double backward of the CPU oracle on six million edges; the 270 901-node run
  prints what its two oracle calls cost (the line ``SCALE ... dense oracle``: 6 s and 4.7 GiB of peak host memory when this
  file was written), both scale linearly with the mesh, so the dense comparison at 1 000 519 nodes fits the budget of a test
  here and is done (measured: 14 s, 13.1 GiB); its own cost is printed the same way.
"""
import resource
import time

import pytest
import torch

import pgrad_ref as pr
from oracle import psignn_oracle as orc
from test_gpu_gradients_at_scale import TAU, _masked, _nonzero, _report, scale  # noqa: F401  (scale: the module's fixture)

pytestmark = pytest.mark.gpu


def _probes(r):
    """Every probe of the 2 N plan-order records must carry a term; parameters tensor by tensor, dh over the support."""
    H, G = r.dev_(r.h), r.dev_(r.gb)
    for name, pos in pr.probes(2 * r.N, seam=r.N).items():
        S = r.support(pr.nodes_at(pos, r.perm, r.N))
        keep, m32, m64 = r.sub(S, 2)
        v = _masked(r.v, torch.from_numpy(S))
        h, h0, vk, gk = r.h[keep], r.h0[keep], v[keep], r.gb[keep]
        want, want_h, _ = orc.function_vjp_backward(r.s64, h.double(), h0.double(), m64, vk.double(), gk.double())
        want32, want32_h, _ = orc.function_vjp_backward(r.sd, h, h0, m32, vk, gk)
        g, dh = r.fm.vjp_backward(H, r.dev_(v), G, tiled=True)
        _nonzero(f"{r.name} vjp_backward tiled probe [{name}]", want)
        r.check_params(f"vjp_backward tiled probe [{name}]", g, want, want32, TAU["jr"])
        r.check_vec(f"vjp_backward tiled probe [{name}] dh", dh, r.scatter(keep, want_h), r.scatter(keep, want32_h), TAU["jr_h"])


def _dense(r):
    """The whole product against the oracle on the whole mesh; the same bits on a second call; the distance to the gather route
    (reported)."""
    H, V, G = r.dev_(r.h), r.dev_(r.v), r.dev_(r.gb)
    t0 = time.time()
    want, want_h, _ = orc.function_vjp_backward(r.s64, r.h.double(), r.h0.double(), r.m64, r.v.double(), r.gb.double())
    want32, want32_h, _ = orc.function_vjp_backward(r.sd, r.h, r.h0, r.m, r.v, r.gb)
    print(f"SCALE {r.name} dense oracle (float64 + float32 double backward): {time.time() - t0:.0f} s, "
          f"peak host memory {resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20:.1f} GiB")
    g, dh = r.fm.vjp_backward(H, V, G, tiled=True)
    assert set(g) == set(want)
    r.check_params("vjp_backward tiled", g, want, want32, TAU["jr"])
    r.check("vjp_backward tiled dh", dh, want_h, want32_h, TAU["jr_h"])
    del want, want_h, want32, want32_h
    g2, dh2 = r.fm.vjp_backward(H, V, G, tiled=True)
    assert all(torch.equal(g[k], g2[k]) for k in g) and torch.equal(dh, dh2)
    gg, dg = r.fm.vjp_backward(H, V, G)
    sc = max(float(t.norm()) for t in gg.values())
    d = max(float((g[k] - gg[k]).double().norm()) / max(float(gg[k].double().norm()), 1e-4 * sc) for k in g)
    print(f"SCALE {r.name} vjp_backward tiled vs gather route: worst tensor {d:.2e}, dh "
          f"{float((dh - dg).double().norm() / dg.double().norm()):.2e}")


def test_tiled_vjp_backward_at_270k(scale):
    r = scale(270901, False)
    assert r.fm.can_tile_vjp_backward()
    _dense(r)
    _probes(r)


def test_tiled_vjp_backward_at_1m(scale):
    """2 001 038 records: a size the backward of the VJP had not been run at."""
    r = scale(1000519, False)
    assert r.fm.can_tile_vjp_backward()
    nblk, npw = pr.pgrad_blocks(2 * r.N)
    assert npw > 64 and 2 * r.N > 262144
    _probes(r)
    _dense(r)
