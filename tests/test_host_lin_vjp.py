"""CPU: the surface of the transposed stored linearisation (no compute calls -- there is no GPU here)."""
import ctypes
import inspect
import os
import re

from conftest import ROOT, pkg

NEW = ("psignn_lin_vjp", "psignn_broyden_solve_adjoint_lin")


def test_linearization_has_vjp_p():
    eng = pkg("engine")
    assert callable(getattr(eng.Linearization, "vjp_p", None))
    assert list(inspect.signature(eng.Linearization.vjp_p).parameters) == ["self", "Wp", "out"]


def test_solve_adjoint_accepts_lin():
    sig = inspect.signature(pkg("engine").DeviceBroyden.solve_adjoint)
    assert "lin" in sig.parameters and sig.parameters["lin"].default is None


def test_model_copies_bw_linearize_only_as_given():
    mp = pkg("model_psignn")
    base = dict(latent_dim=10, n_layers=1)
    net = mp.ModelDEQDSS(base)
    assert "bw_linearize" not in net.deqdss.config_deq
    assert net.deqdss._linearize_default(None) is False
    on = mp.ModelDEQDSS(dict(base, bw_linearize=True))
    assert on.deqdss.config_deq["bw_linearize"] is True and on.deqdss._linearize_default(None) is True
    assert on.deqdss._linearize_default(False) is False and net.deqdss._linearize_default(True) is True
    off = pkg("mixed").ModelDEQDSS(dict(base, bw_linearize=False))
    assert off.deqdss.config_deq["bw_linearize"] is False
    for meth in ("power_method", "jac_loss_estimate"):
        p = inspect.signature(getattr(mp.DeepEquilibrium, meth)).parameters
        assert "linearize" in p and p["linearize"].default is None


def test_new_symbols_declared_exported_bound():
    nat = pkg("_native")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "psignn_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW:
        m = re.search(r"\b" + name + r"\s*\(([^()]*)\)\s*;", hdr)
        assert m, name
        assert hasattr(lib, name), name
        assert name in nat.SIGNATURES and len(nat.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
