"""CPU: the surface of the multi-layer dirichlet derivatives (no compute calls -- there is no GPU here)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT, pkg

NEW = ("psignn_f_jvp_pw", "psignn_f_layers_workspace_floats", "psignn_f_param_vjp_ex")


def test_new_symbols_declared_exported_bound():
    nat = pkg("_native")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "psignn_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW:
        m = re.search(r"\b" + name + r"\s*\(([^()]*)\)\s*;", hdr)
        assert m, name
        assert hasattr(lib, name), name
        assert name in nat.SIGNATURES and len(nat.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name


def test_layer_workspace_query_rejects_bad_arguments():
    """NULL plan and depths outside 1..64 are refused with -1 before any plan field is read."""
    lib = pkg("_native").lib()
    assert lib.psignn_f_layers_workspace_floats(None, 2) == -1
    assert lib.psignn_f_layers_workspace_floats(None, 0) == -1


@pytest.mark.parametrize("mixed", [False, True])
def test_unpack_param_grads_names_every_layer(mixed):
    """Names and shapes at L = 1, 2, 3; the named slices are disjoint, inside psignn_param_grad_size, and layer k's section
    starts k layer sizes after layer 0's."""
    eng, nat = pkg("engine"), pkg("_native")
    lib = nat.lib()
    lsz = int(lib.psignn_param_grad_size(int(mixed), 2)) - int(lib.psignn_param_grad_size(int(mixed), 1))
    one = None
    for L in (1, 2, 3):
        n = int(lib.psignn_param_grad_size(int(mixed), L))
        flat = torch.arange(n, dtype=torch.float64)
        g = eng.unpack_param_grads(flat, L, mixed)
        expect = {"laynorm.weight", "laynorm.bias", "alpha.0.weight", "alpha.0.bias"}
        for k in range(L):
            for phi in ("phi_to_list", "phi_from_list"):
                expect |= {f"{phi}.{k}.mlp.mlp.{i}.{t}" for i in (0, 2) for t in ("weight", "bias")}
            expect |= {f"update_list.{k}.mlp.{i}.{t}" for i in (0, 2) for t in ("weight", "bias")}
        if mixed:
            expect |= {f"phi_neumann.mlp.mlp.{i}.{t}" for i in (0, 2) for t in ("weight", "bias")}
            expect |= {f"update_neumann.mlp.{i}.{t}" for i in (0, 2) for t in ("weight", "bias")}
        assert set(g) == expect
        idx = torch.cat([t.reshape(-1) for t in g.values()]).long()
        assert len(set(idx.tolist())) == idx.numel() and int(idx.max()) < n
        if one is None:
            one = g
        for k in range(L):
            for name, t in one.items():
                if "_list.0." in name:
                    assert torch.equal(g[name.replace("_list.0.", f"_list.{k}.")], t + k * lsz), (L, k, name)
                elif "neumann" in name:
                    assert torch.equal(g[name], t + (L - 1) * lsz)
                else:
                    assert torch.equal(g[name], t)
    with pytest.raises(nat.NativeError):
        eng.unpack_param_grads(torch.zeros(5), 2, mixed)


def test_train_forward_reaches_the_device_at_two_layers():
    """n_layers = 2 is no longer refused on the host: the training forward gets as far as the device (none here)."""
    nat = pkg("_native")
    mesh = pkg("data").make_hex_problem(3, seed=0)
    net = pkg("model_psignn").ModelPSIGNN(dict(latent_dim=10, n_layers=2)).train()
    with pytest.raises(nat.NativeError) as e:
        net(mesh)
    assert "single-layer" not in str(e.value)
