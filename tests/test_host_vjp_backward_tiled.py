"""CPU: the surface of the tile form of the backward of the VJP (no compute calls -- there is no GPU here)."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT, pkg

NEW = {"psignn_f_vjp_backward_tiled_ok": 2, "psignn_f_vjp_backward_p_workspace_floats": 1, "psignn_f_vjp_backward_p": 11}


def test_new_symbols_declared_exported_bound():
    nat = pkg("_native")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "psignn_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name, arity in NEW.items():
        m = re.search(r"\b" + name + r"\s*\(([^()]*)\)\s*;", hdr)
        assert m, name
        assert m.group(1).count(",") + 1 == arity, name
        assert hasattr(lib, name), name
        assert name in nat.SIGNATURES and len(nat.SIGNATURES[name][1]) == arity, name


def test_tiled_ok_is_zero_without_a_plan():
    lib = pkg("_native").lib()
    assert lib.psignn_f_vjp_backward_tiled_ok(None, 1) == 0
    assert lib.psignn_f_vjp_backward_p_workspace_floats(None) == 0


def test_python_surface():
    eng = pkg("engine")
    p = inspect.signature(eng.FixedPointMap.vjp_backward).parameters
    assert list(p) == ["self", "H", "V", "Gbar", "tiled"] and p["tiled"].default is False
    assert list(inspect.signature(eng.FixedPointMap.vjp_backward_p).parameters) == ["self", "Hp", "Vp", "Gp"]
    assert callable(eng.FixedPointMap.can_tile_vjp_backward)
    assert eng.FixedPointMap.jac_backward == "gather"
    for ok in ("gather", "tiled"):
        assert eng.check_jac_backward(ok) == ok
    for bad in ("bogus", "", "Tiled", None, 1, True):
        with pytest.raises(ValueError):
            eng.check_jac_backward(bad)


def test_model_reads_jac_backward():
    mp = pkg("model_psignn")
    base = dict(latent_dim=10, n_layers=1)
    for mod in (mp, pkg("mixed")):
        net = mod.ModelDEQDSS(base)
        assert "jac_backward" not in net.deqdss.config_deq and net.deqdss.f.jac_backward == "gather"
        on = mod.ModelDEQDSS(dict(base, jac_backward="tiled"))
        assert on.deqdss.config_deq["jac_backward"] == "tiled" and on.deqdss.f.jac_backward == "tiled"
        off = mod.ModelPSIGNN(dict(base, jac_backward="gather"))
        assert off.deqdss.config_deq["jac_backward"] == "gather" and off.deqdss.f.jac_backward == "gather"
        for bad in ("bogus", None, 1):
            with pytest.raises(ValueError):
                mod.ModelDEQDSS(dict(base, jac_backward=bad))
