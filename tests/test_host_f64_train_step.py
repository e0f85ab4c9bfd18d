"""CPU: the float64 losses and the one-call float64 training step (``psignn_residual_f64``, ``psignn_residual_t_f64``,
``psignn_mse_f64`` and its queries; ``engine.residual64``, ``residual64_t``, ``mse64``, ``train_step64``) -- the C ABI surface, every
refusal that needs no device, and the CPU restatement the GPU tests compare against.

``train_step_ref`` (tests/train_step_ref.py) at ``orc.training_step``'s own ``out_fw["result"]`` / ``out_bw["result"]`` builds the same
autograd graph as the oracle.  scripts/calib_f64_train_step.py measured the two against each other on the three fixtures and the two
two-layer blocks (float64, ``jac_weight`` 1, one seeded probe): every gradient tensor, every loss term and the loss are bit-equal
(0.0e+00 in every case), so the gate here is equality -- tighter than the 5.5e-15 a by-hand composition of the same formulas reaches."""
import ctypes
import inspect
import math
import os
import re
import types

import pytest
import torch

import train_step_ref as ts
from conftest import ROOT, load_weights, pkg

LOSS_CITES = ("157-167", "58-99")   # model.py:157-167 (residual_loss) and model.py:58-99 (ModelDEQDSS.forward)
NEW = {"psignn_residual_f64": (6, LOSS_CITES), "psignn_residual_t_f64": (5, LOSS_CITES), "psignn_mse_f64_chunk": (0, LOSS_CITES),
       "psignn_mse_f64_workspace_doubles": (1, LOSS_CITES), "psignn_mse_f64": (9, LOSS_CITES),
       "psignn_f64_vjp_backward_init": (16, ("416-435", "184-207"))}


def test_entries_in_header_table_and_default_library_only():
    nat = pkg("_native")
    raw_hdr = open(os.path.join(ROOT, "include", "psignn_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw_hdr, flags=re.S)
    decl = dict(re.findall(r"\b(psignn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr))
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name, (arity, cites) in NEW.items():
        assert name in decl, name
        params = decl[name].strip()
        assert (0 if params in ("", "void") else params.count(",") + 1) == arity, (name, decl[name])
        assert len(nat.SIGNATURES[name][1]) == arity, name
        assert hasattr(lib, name), name
        # the comment in front of the declaration carries a replaces: line citing the reference
        head = raw_hdr[:re.search(r"^(int|int64_t) " + name + r"\(", raw_hdr, re.M).start()]
        comment = head[head.rindex("/*"):]
        assert "replaces:" in comment and "model.py" in comment and all(c in comment for c in cites), name
    for w in (8, 16):   # default-width library only
        raw = ctypes.CDLL(nat.lib_path(w))
        assert not any(hasattr(raw, n) for n in NEW), w


def test_every_entry_has_an_integration_row_citing_the_reference():
    rows = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if l.startswith("|")]
    for name, (_, cites) in NEW.items():
        hits = [l for l in rows if name in l]
        assert hits and any(any("model.py:" + c in l for c in cites) for l in hits), name


def test_the_kernels_live_in_a_unit_of_the_default_library_only():
    """Beside the float64 solve of the same system, in a unit that already shares f64_common.h; no atomics; the plan's fp32 copy of
    a_ij is read nowhere in it."""
    mk = open(os.path.join(ROOT, "psi-gnn_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    fwd = re.search(r"^FWD_SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "poisson_cg.hip" in srcs and "poisson_cg.hip" not in fwd
    text = open(os.path.join(ROOT, "psi-gnn_amd", "csrc", "poisson_cg.hip")).read()
    assert '#include "f64_common.h"' in text
    new = text[text.index("// The losses of a training step in float64"):]   # the section this change adds, to the end of the file
    assert all(k in new for k in ("k_residual_f64", "k_residual_t_f64", "k_mse_f64", "k_mse_f64_final"))
    assert "atomic" not in new.replace("No atomics", "")
    assert "a_val" not in new   # the plan's fp32 copy of a_ij is not read


def test_python_signatures():
    eng = pkg("engine")
    sig = lambda f: inspect.signature(f).parameters
    assert list(sig(eng.residual64)) == ["plan", "a_ij", "u", "y"]
    assert list(sig(eng.residual64_t)) == ["plan", "a_ij", "r"]
    assert list(sig(eng.FixedPointMap64.vjp_backward_init)) == list(sig(eng.FixedPointMap64.vjp_backward)) == ["self", "H", "V", "Gbar"]
    p = sig(eng.mse64)
    assert list(p) == ["a", "b", "need_grad"] and p["b"].default is None and p["need_grad"].default is False
    p = sig(eng.train_step64)
    assert list(p) == ["batch", "state_dict", "h_star", "y", "jac_weight", "probe", "fw_eps", "fw_threshold", "solver", "eps", "m",
                       "max_products", "threshold"]
    assert [p[k].default for k in list(p)[2:]] == [None, None, 0.0, None, 1e-11, 1000, "gmres", 1e-11, 50, 2000, 800]


def test_queries_and_native_refusals_without_a_device():
    lib = pkg("_native").lib()
    chunk = lib.psignn_mse_f64_chunk()
    assert chunk == 1024
    q = lib.psignn_mse_f64_workspace_doubles
    assert q(0) == -1 and q(-5) == -1
    assert [q(n) for n in (1, chunk - 1, chunk, chunk + 1, 256 * chunk + 1)] == [1, 1, 1, 2, 257]
    err = lambda: lib.psignn_last_error().decode()
    assert lib.psignn_mse_f64(None, None, 4, 4.0, None, None, None, 0, None) < 0 and "NULL" in err()
    assert lib.psignn_mse_f64(8, None, 0, 1.0, 16, None, 24, 1, None) < 0 and "n_elems" in err()   # refused before a pointer is read
    assert lib.psignn_mse_f64(8, None, 4, 0.0, 16, None, 24, 1, None) < 0 and "scale_n" in err()
    assert lib.psignn_mse_f64(8, None, 4, 4.0, 16, 8, 24, 1, None) < 0 and "alias" in err()
    assert lib.psignn_mse_f64(8, 32, 4, 4.0, 16, 32, 24, 1, None) < 0 and "alias" in err()
    assert lib.psignn_mse_f64(8, None, 4, 4.0, 8, None, 24, 1, None) < 0 and "alias" in err()
    assert lib.psignn_mse_f64(8, None, 2 * chunk, 4.0, 16, None, 24, 1, None) < 0 and f"{2 * 8} bytes" in err()
    assert lib.psignn_mse_f64(8, None, 4, 4.0, 16, None, None, 1, None) < 0 and "8 bytes" in err()
    assert lib.psignn_residual_f64(None, None, None, None, None, None) < 0 and "NULL" in err()
    assert lib.psignn_residual_t_f64(None, None, None, None, None) < 0 and "NULL" in err()
    assert lib.psignn_f64_vjp_backward_init(None, None, 1, None, None, None, None, None, None, None, None, None, None, None, 0, None) < 0
    assert "NULL" in err() and "psignn_f64_vjp_backward_init" in err()


def _plan(N=7, E=20):
    return types.SimpleNamespace(mixed=False, N=N, E=E, device=torch.device("cpu"), handle=None)


def test_residual64_and_mse64_refusals_without_a_device():
    nat, eng = pkg("_native"), pkg("engine")
    plan = _plan()
    a, u = torch.zeros(20, 1), torch.zeros(7, 1)
    for bad in (torch.zeros(6, 1), torch.zeros(7, 2), torch.zeros(7, 1, 1), torch.zeros(8)):
        with pytest.raises(nat.NativeError, match="u has shape"):
            eng.residual64(plan, a, bad, u)
        with pytest.raises(nat.NativeError, match="y has shape"):
            eng.residual64(plan, a, u, bad)
        with pytest.raises(nat.NativeError, match="r has shape"):
            eng.residual64_t(plan, a, bad)
    for bad in (torch.zeros(19), torch.zeros(21, 1), torch.zeros(0)):
        with pytest.raises(nat.NativeError, match="a_ij has"):
            eng.residual64(plan, bad, u.double().reshape(-1), u)   # refused on the host: nothing is on a device here
    with pytest.raises(nat.NativeError, match="empty"):
        eng.residual64(_plan(0, 0), torch.zeros(0), torch.zeros(0, 1), torch.zeros(0, 1))
    with pytest.raises(nat.NativeError, match="device tensors"):   # shapes right, tensors on the host: there is no CPU route
        eng.residual64(plan, a, u, u)
    with pytest.raises(nat.NativeError, match="device tensors"):
        eng.residual64_t(plan, a, u)
    with pytest.raises(nat.NativeError, match="b "):
        eng.mse64(torch.zeros(4, 2), torch.zeros(4, 3))
    with pytest.raises(nat.NativeError, match="empty"):
        eng.mse64(torch.zeros(0, 3))
    with pytest.raises(nat.NativeError, match="device tensors"):
        eng.mse64(torch.zeros(4, 2), None, need_grad=True)


def test_train_step64_refusals_without_a_device():
    nat, eng = pkg("_native"), pkg("engine")
    sd = load_weights("dirichlet")
    batch = types.SimpleNamespace(x=torch.zeros(7, 1))
    ok = torch.zeros(7, 10)
    for w in (8, 16):   # a state dict of another latent width: forward inference only
        wide = {"deqdss.f.laynorm.weight": torch.zeros(w)}
        with pytest.raises(nat.NativeError, match="forward inference only"):
            eng.train_step64(batch, wide, h_star=ok, y=ok)
    with pytest.raises(nat.NativeError, match="needs a probe"):
        eng.train_step64(batch, sd, h_star=ok, y=ok, jac_weight=1.0)
    with pytest.raises(nat.NativeError, match="solver must be"):
        eng.train_step64(batch, sd, h_star=ok, y=ok, solver="anderson")
    for bad in (torch.zeros(7, 8), torch.zeros(6, 10)):
        with pytest.raises(nat.NativeError, match="h_star has shape"):
            eng.train_step64(batch, sd, h_star=bad, y=ok)
        with pytest.raises(nat.NativeError, match="y has shape"):
            eng.train_step64(batch, sd, h_star=ok, y=bad)
        with pytest.raises(nat.NativeError, match="probe has shape"):
            eng.train_step64(batch, sd, h_star=ok, y=ok, probe=bad, jac_weight=1.0)
    with pytest.raises(nat.NativeError, match="device tensors"):   # everything in order, tensors on the host: no CPU route
        eng.train_step64(batch, sd, h_star=ok, y=ok, probe=ok, jac_weight=1.0)


def test_train_step_ref_is_the_oracle_step_at_its_own_state():
    """hex13_mixed_s1, float64, ``jac_weight`` 1 (about a second; the dirichlet fixtures take longer and are measured by the
    calibration script): the same graph, so the same bits."""
    o = ts.oracle_at("hex13_mixed_s1")
    assert o["fw"]["lowest"] < 1e-11 and o["bw"]["lowest"] < 1e-11
    hs, y = o["fw"]["result"].detach(), o["bw"]["result"].detach()
    loss, dic, grads, grad_h = ts.train_step_ref(o["sd"], o["mesh"], hs, y, o["probe"], 1.0)
    assert set(grads) == set(o["grads"]) == set(o["sd"]) and list(dic) == ts.LOSS_KEYS
    for k, t in o["grads"].items():
        assert grads[k].dtype == torch.float64 and torch.equal(grads[k], t), (k, ts.rel(grads[k], t))
    for k, v in o["loss_dic"].items():
        assert float(dic[k]) == float(v), (k, float(dic[k]), float(v))
    assert float(loss) == float(o["loss"]) and math.isfinite(float(loss))
    assert grad_h.shape == hs.shape and bool(grad_h.any())
    # the float32 value of the same code: close to the float64 one, not equal to it
    l32, d32, g32, _ = ts.train_step_ref(o["sd"], o["mesh"], hs, y, o["probe"], 1.0, dtype=torch.float32)
    assert all(t.dtype == torch.float32 for t in g32.values())
    assert 0 < abs(float(l32) - float(loss)) < 1e-3 * float(loss)
