"""CPU: the surface of the stored linearisation's Neumann option (no compute calls -- there is no GPU here)."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT, pkg

NEW = ("psignn_lin_create_opts", "psignn_lin_neumann_stored")


def test_new_symbols_declared_exported_bound():
    nat = pkg("_native")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "psignn_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name, arity in zip(NEW, (3, 1)):
        m = re.search(r"\b" + name + r"\s*\(([^()]*)\)\s*;", hdr)
        assert m, name
        assert m.group(1).count(",") + 1 == arity, name
        assert hasattr(lib, name), name
        assert name in nat.SIGNATURES and len(nat.SIGNATURES[name][1]) == arity, name


class _NoLibrary:
    """Stands in for a FixedPointMap: any use beyond the argument check fails the test."""
    lin_neumann = "direct"
    _p = None

    def __getattr__(self, name):
        raise AssertionError(f"the map was touched ({name}) before neumann= was checked")


def test_neumann_argument_is_checked_on_the_host(monkeypatch):
    eng, nat = pkg("engine"), pkg("_native")
    p = inspect.signature(eng.Linearization.__init__).parameters
    assert list(p) == ["self", "fmap", "neumann"] and p["neumann"].default == "direct"
    p = inspect.signature(eng.FixedPointMap.linearize_p).parameters
    assert list(p) == ["self", "Hp", "lin", "neumann"] and p["lin"].default is None
    assert eng.FixedPointMap.lin_neumann == "direct"            # what neumann=None resolves to unless the map says otherwise
    monkeypatch.setattr(nat, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    for bad in ("bogus", "", "Stored", 1, True):
        with pytest.raises(ValueError):
            eng.Linearization(_NoLibrary(), neumann=bad)
        with pytest.raises(ValueError):
            eng.FixedPointMap.linearize_p(_NoLibrary(), None, neumann=bad)
    for ok in ("direct", "stored"):
        assert eng.check_lin_neumann(ok) == ok


def test_model_reads_lin_neumann():
    mp = pkg("model_psignn")
    base = dict(latent_dim=10, n_layers=1)
    for mod in (mp, pkg("mixed")):
        net = mod.ModelDEQDSS(base)
        assert "lin_neumann" not in net.deqdss.config_deq and net.deqdss.f.lin_neumann == "direct"
        on = mod.ModelDEQDSS(dict(base, bw_linearize=True, lin_neumann="stored"))
        assert on.deqdss.config_deq["lin_neumann"] == "stored" and on.deqdss.f.lin_neumann == "stored"
        off = mod.ModelPSIGNN(dict(base, lin_neumann="direct"))
        assert off.deqdss.config_deq["lin_neumann"] == "direct" and off.deqdss.f.lin_neumann == "direct"
        for bad in ("bogus", None, 1):
            with pytest.raises(ValueError):
                mod.ModelDEQDSS(dict(base, lin_neumann=bad))
