"""CPU: the surface of the batched adjoint solve and of the replica route (C ABI, ctypes table, Python entry points,
``DataParallel(..., replicas=)``); no compute calls -- there is no GPU here."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT, pkg


def test_batched_adjoint_symbols_declared_exported_bound():
    nat = pkg("_native")
    hdr = open(os.path.join(ROOT, "include", "psignn_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = dict(re.findall(r"\b(psignn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr))
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name, nargs in (("psignn_broyden_adjoint_batchable", 3), ("psignn_broyden_solve_adjoint_lin_batch", 13)):
        assert name in decl, name
        assert decl[name].count(",") + 1 == nargs
        assert hasattr(lib, name)
        assert len(nat.SIGNATURES[name][1]) == nargs
    # a host-side question: 0 for an empty shard and for NULL arguments, nothing touched
    L = nat.lib()
    assert L.psignn_broyden_adjoint_batchable(0, None, None) == 0
    assert L.psignn_broyden_adjoint_batchable(2, None, None) == 0
    one = (ctypes.c_void_p * 1)(None)
    assert L.psignn_broyden_adjoint_batchable(1, one, None) == 0
    assert L.psignn_broyden_adjoint_batchable(1, one, one) == 0


def test_integration_table_names_both_entries():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("psignn_broyden_adjoint_batchable", "psignn_broyden_solve_adjoint_lin_batch"):
        row = [ln for ln in doc.splitlines() if ln.startswith("|") and name in ln]
        assert row, name
        assert "main.py:106" in row[0] and "model.py:210-223" in row[0]


def test_python_surface():
    eng, model, loader = pkg("engine"), pkg("model_psignn"), pkg("loader")
    assert list(inspect.signature(eng.adjoint_batchable).parameters) == ["solvers", "lins"]
    sig = inspect.signature(eng.broyden_solve_adjoint_batch)
    assert list(sig.parameters) == ["solvers", "lins", "grads", "eps", "poll_every"]
    assert sig.parameters["poll_every"].default == 8
    assert eng.adjoint_batchable([], []) is False
    assert eng.broyden_solve_adjoint_batch([], [], [], 1e-6) == []
    sig = inspect.signature(model.DeepEquilibrium.train_forward_replicas)
    assert list(sig.parameters) == ["self", "H_inits", "batches", "generator"]
    assert sig.parameters["generator"].default is None
    sig = inspect.signature(loader.DataParallel.__init__)
    assert list(sig.parameters) == ["self", "module", "device_ids", "output_device", "replicas"]
    assert sig.parameters["replicas"].default == 1


class Probe(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, batch):
        if isinstance(batch, (list, tuple)):
            return [(b.num_nodes, getattr(b, "num_graphs", 1), b) for b in batch]
        return batch.num_nodes, getattr(batch, "num_graphs", 1)


def test_data_parallel_replicas_chunks():
    data, loader = pkg("data"), pkg("loader")
    ds = [data.make_hex_problem(3, seed=s) for s in range(5)]
    n0 = ds[0].num_nodes
    out = loader.DataParallel(Probe(), replicas=2)(ds)
    assert [(n, g) for n, g, _ in out] == [(3 * n0, 3), (2 * n0, 2)]
    # contiguous, in order: the chunks' node data are the graphs' in the list's order
    want = [torch.cat([g.x for g in ds[:3]]), torch.cat([g.x for g in ds[3:]])]
    assert all(torch.equal(b.x, w) for (_, _, b), w in zip(out, want))
    out = loader.DataParallel(Probe(), replicas=8)(ds)
    assert [(n, g) for n, g, _ in out] == [(n0, 1)] * 5
    assert all(torch.equal(b.x, g.x) for (_, _, b), g in zip(out, ds))
    out = loader.DataParallel(Probe(), replicas=3)(ds)
    assert [g for _, g, _ in out] == [2, 2, 1]
    # replicas = 1 and the default: one union batch, the values of test_loader_stand_ins
    for dp in (loader.DataParallel(Probe()), loader.DataParallel(Probe(), replicas=1)):
        assert dp.module is not None
        assert dp([ds[0]]) == (n0, 1)
        assert dp(ds[:3]) == (3 * n0, 3)
    for bad in (0, -2):
        with pytest.raises(ValueError):
            loader.DataParallel(Probe(), replicas=bad)
