"""CPU: the opt-in GMRES adjoint solve (``bw_solver = "gmres"``) -- its C ABI surface, the host-side checks of its config keys,
and the algorithm itself as a torch restatement (tests/adjoint_gmres_ref.py) on the CPU oracle's VJP.

Gates of the algorithm test, all from the issue: on the three stored fixtures, float32 vectors, restart length 50, tolerance 1e-8
and a budget of 500 products (the launch configuration of the reference's backward), the solve stops by stagnation or tolerance,
spends fewer products than the oracle's fp32 Broyden on the same system, and its error against the float64 adjoint is at most
twice that Broyden's (both sit at the fp32 floor, where the ratio scatters around 1)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT, pkg

NEW = {"psignn_gmres_adjoint_workspace_floats": 2, "psignn_gmres_solve_adjoint": 17, "psignn_gmres_solve_adjoint_lin": 14}


def test_new_entries_in_header_table_and_library():
    nat = pkg("_native")
    hdr = open(os.path.join(ROOT, "include", "psignn_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = dict(re.findall(r"\b(psignn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr))
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name, arity in NEW.items():
        assert name in decl, name
        assert decl[name].count(",") + 1 == arity, (name, decl[name])
        assert len(nat.SIGNATURES[name][1]) == arity, name
        assert hasattr(lib, name), name
    assert nat.SIGNATURES["psignn_gmres_adjoint_workspace_floats"][0] is ctypes.c_int64
    assert "psignn_gmres_adjoint_info_t" in hdr
    assert [f for f, _ in nat.GmresAdjointInfo._fields_] == ["products", "cycles", "stop_reason", "n_reorth", "lowest", "lowest_abs"]
    assert ctypes.sizeof(nat.GmresAdjointInfo) == 32
    # the width libraries hold no derivatives: the new entries are not in them
    for w in (8, 16):
        raw = ctypes.CDLL(nat.lib_path(w))
        assert not any(hasattr(raw, n) for n in NEW)
    # pure host queries answer bad arguments with -1
    assert nat.lib().psignn_gmres_adjoint_workspace_floats(None, 1) == -1


def test_check_bw_solver():
    eng, nat = pkg("engine"), pkg("_native")
    assert eng.check_bw_solver(None) is None
    assert eng.check_bw_solver("gmres") == "gmres"
    for bad in ("broyden", "GMRES", "", 1, True, ("gmres",)):
        with pytest.raises(nat.NativeError, match=r"bw_solver must be one of \(None, 'gmres'\)"):
            eng.check_bw_solver(bad)
    assert eng.check_bw_solver("gmres", 2, 500) == "gmres" and eng.check_bw_solver("gmres", 500, 500) == "gmres"
    for bad in (1, 0, -3, 501, 2.0, "50", True):
        with pytest.raises(nat.NativeError, match=r"bw_gmres_m must be an int in 2\.\.bw_thres \(= 500\)"):
            eng.check_bw_solver("gmres", bad, 500)


def test_model_config_keys():
    nat = pkg("_native")
    mk = lambda **kw: pkg("model_psignn").ModelDEQDSS(dict(latent_dim=10, n_layers=1, bw_thres=40, **kw))
    assert "bw_solver" not in mk().config_deq and "bw_gmres_m" not in mk().config_deq
    net = mk(bw_solver=None)
    assert net.config_deq["bw_solver"] is None
    net = mk(bw_solver="gmres")
    assert net.config_deq["bw_solver"] == "gmres" and net.config_deq["bw_gmres_m"] == 40   # (default 50, at most bw_thres)
    assert mk(bw_solver="gmres", bw_gmres_m=7).config_deq["bw_gmres_m"] == 7
    with pytest.raises(nat.NativeError, match="bw_solver must be one of"):
        mk(bw_solver="anderson")
    for m in (1, 41):
        with pytest.raises(nat.NativeError, match="bw_gmres_m must be an int in 2..bw_thres"):
            mk(bw_solver="gmres", bw_gmres_m=m)
    # the mixed family's model takes the same keys
    assert pkg("mixed").ModelDEQDSS(dict(latent_dim=10, n_layers=1, bw_solver="gmres")).config_deq["bw_gmres_m"] == 50
    # replicas with the key never take the lockstep route (decided on the host, before the maps are looked at)
    assert mk(bw_solver="gmres", bw_gmres_m=7).deqdss.lockstep_applies([object()]) is False


@pytest.mark.parametrize("d", [8, 16])
def test_other_widths_stay_forward_only_with_the_key(d, monkeypatch):
    nat = pkg("_native")
    net = pkg("model_psignn").ModelDEQDSS(dict(latent_dim=d, n_layers=1, bw_solver="gmres"))
    monkeypatch.setattr(nat, "lib", lambda *a: (_ for _ in ()).throw(AssertionError("the library was touched")))
    deq = net.deqdss
    for call in (lambda: net.train()(object()), lambda: deq.train_forward(torch.zeros(3, d), object()),
                 lambda: deq.implicit_backward(None, None, object(), torch.zeros(3, d)),
                 lambda: deq.train_forward_replicas([torch.zeros(3, d)], [object()])):
        with pytest.raises(nat.NativeError, match=f"latent_dim {d} has forward inference only"):
            call()


@pytest.mark.parametrize("name", ["hex13_dirichlet_s0", "hex26_dirichlet_s0", "hex13_mixed_s1"])
def test_cycle_logic_on_the_oracle_vjp(name):
    import adjoint_gmres_ref as ref
    P = ref.AdjointProblem(name)
    bro, bro_products = P.broyden32(eps=1e-8, threshold=500)
    out = ref.gmres_adjoint(P.vjp32, P.grad, 1e-8, 500, m=50)
    e_gm, e_br = P.error(out["result"]), P.error(bro["result"])
    print(f"ADJOINT_GMRES_REF {name}: GMRES(50) products {out['nstep']} cycles {out['n_cycles']} stop {out['stop']} "
          f"lowest {out['lowest']:.2e} error {e_gm:.2e} | Broyden products {bro_products} lowest {bro['lowest']:.2e} error {e_br:.2e}")
    assert out["stop"] in ("stagnation", "tolerance"), out["stop"]
    assert out["nstep"] < bro_products, (out["nstep"], bro_products)
    assert e_gm <= 2.0 * e_br, (e_gm, e_br)
    # the dict is self-consistent: one trace entry per cycle, lowest is the smallest of them and belongs to the result
    assert len(out["rel_trace"]) == len(out["abs_trace"]) == out["n_cycles"] and out["lowest"] == min(out["rel_trace"])
    f = P.vjp32(out["result"]) + P.grad
    assert abs(float((f - out["result"]).norm() / (f.norm() + 1e-9)) - out["lowest"]) <= 1e-3 * out["lowest"]
