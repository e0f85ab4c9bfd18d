"""CPU: the C ABI and Python surface of the bf16 Broyden pair history (no device is touched)."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT, pkg


def test_create_opts_is_declared_and_bound():
    nat = pkg("_native")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "psignn_hip.h")).read(), flags=re.S)
    m = re.search(r"\bpsignn_broyden_create_opts\s*\(([^()]*)\)\s*;", hdr)
    assert m and m.group(1).count(",") + 1 == 8
    assert len(nat.SIGNATURES["psignn_broyden_create_opts"][1]) == 8
    assert "psignn_broyden_create_opts" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # an unknown history kind is refused before anything is allocated
    h = C.c_void_p()
    for hist in (2, -1):
        assert nat.lib().psignn_broyden_create_opts(C.byref(h), None, 1000, 10, 20, 0, 0, hist) != 0
        assert not h.value


def test_other_history_dtypes_are_refused_on_the_host():
    eng, solver, model = pkg("engine"), pkg("utilities.solver"), pkg("model_psignn")
    assert eng.history_code(torch.float32) == 0 and eng.history_code(torch.bfloat16) == 1
    with pytest.raises(ValueError):
        eng.DeviceBroyden(threshold=10, n_elems=100, device=torch.device("cuda:0"), history_dtype=torch.float16)
    with pytest.raises(ValueError):
        solver.broyden(lambda x: x, torch.zeros(10, 10), threshold=10, history_dtype=torch.float16)
    with pytest.raises(ValueError):
        model.ModelDEQDSS(dict(latent_dim=10, n_layers=1, broyden_history_dtype=torch.float16))
    # the accepted dtypes reach the solver configuration
    net = model.ModelDEQDSS(dict(latent_dim=10, n_layers=1, broyden_history_dtype=torch.bfloat16))
    assert net.deqdss.history_dtype() == torch.bfloat16 and net.deqdss._solver_kwargs() == {"history_dtype": torch.bfloat16}
    net = model.ModelDEQDSS(dict(latent_dim=10, n_layers=1))
    assert net.deqdss.history_dtype() == torch.float32 and net.deqdss._solver_kwargs() == {}
    # with another solver the key has no effect
    net = model.ModelDEQDSS(dict(latent_dim=10, n_layers=1, solver=solver.anderson, broyden_history_dtype=torch.bfloat16))
    assert net.deqdss._solver_kwargs() == {}
