"""CPU: the surface of the latent widths other than 10 (libpsignn_hip_d8.so / _d16.so) -- model shapes, weight packing against
each library's own layout total, the ``psignn_latent_dim`` entry, and the refusals.  No compute calls: there is no GPU here."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT, pkg

WIDTHS = (8, 16)


def _mod(mixed):
    return pkg("mixed") if mixed else pkg("model_psignn")


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("mixed", [False, True])
def test_model_has_the_reference_shapes_and_loads_strictly(d, mixed):
    """dirichlet/psignn/model.py:265-277 (mixed/psignn/model.py:198-214) at latent_dim d."""
    P = 3 if mixed else 2
    net = _mod(mixed).ModelPSIGNN(dict(latent_dim=d, n_layers=1))
    sd = net.state_dict()
    want = {"deqdss.f.laynorm.weight": (d,), "deqdss.f.laynorm.bias": (d,),
            "deqdss.f.alpha.0.weight": (1, 3 * d + P), "deqdss.f.alpha.0.bias": (1,),
            "deqdss.f.update_list.0.mlp.0.weight": (d, 3 * d + P), "deqdss.f.update_list.0.mlp.0.bias": (d,),
            "deqdss.f.update_list.0.mlp.2.weight": (d, d), "deqdss.f.update_list.0.mlp.2.bias": (d,),
            "autoencoder.encoder.mlp.mlp.0.weight": (d, 1), "autoencoder.encoder.mlp.mlp.2.weight": (d, d),
            "autoencoder.decoder.mlp.mlp.0.weight": (d, d), "autoencoder.decoder.mlp.mlp.2.weight": (1, d)}
    phis = ["phi_to_list.0", "phi_from_list.0"] + (["phi_neumann"] if mixed else [])
    for phi in phis:
        want.update({f"deqdss.f.{phi}.mlp.mlp.0.weight": (d, 2 * d + 3), f"deqdss.f.{phi}.mlp.mlp.0.bias": (d,),
                     f"deqdss.f.{phi}.mlp.mlp.2.weight": (d, d), f"deqdss.f.{phi}.mlp.mlp.2.bias": (d,)})
    if mixed:
        want.update({"deqdss.f.update_neumann.mlp.0.weight": (d, 2 * d + P + 2), "deqdss.f.update_neumann.mlp.2.weight": (d, d)})
    for k, shape in want.items():
        assert tuple(sd[k].shape) == shape, (k, tuple(sd[k].shape), shape)
    ref_keys = {k for k in want} | {k.replace(".weight", ".bias") for k in want}
    assert set(sd) == ref_keys, sorted(set(sd) ^ ref_keys)
    for cls in ("ModelPSIGNN", "ModelPSIGNNIterative", "ModelDEQDSS"):
        other = getattr(_mod(mixed), cls)(dict(latent_dim=d, n_layers=1))
        other.load_state_dict(sd, strict=True)
        assert all(torch.equal(v, other.state_dict()[k]) for k, v in sd.items())
    with pytest.raises(RuntimeError):      # a checkpoint of another width does not load
        _mod(mixed).ModelPSIGNN(dict(latent_dim=10, n_layers=1)).load_state_dict(sd, strict=True)


@pytest.mark.parametrize("d", WIDTHS + (10,))
def test_packed_length_is_the_library_total(d):
    """engine.pack_weights computes WLayout from the width; each library reports its own total (n_layers 1 and 2, both families)."""
    eng, nat = pkg("engine"), pkg("_native")
    lib = nat.lib(d)
    rup = lambda n, k: (n + k - 1) // k * k
    for mixed in (False, True):
        P = 3 if mixed else 2
        for nl in (1, 2):
            torch.manual_seed(5)
            sd = _mod(mixed).ModelPSIGNN(dict(latent_dim=d, n_layers=nl)).state_dict()
            flat = eng.pack_weights(sd)
            phi = d * (2 * d + 3) + d + d * d + d
            layer = 2 * phi + (d * (3 * d + P) + d + d * d + d) + rup(2 * d * d + 4 * d + 2, 4)
            total = rup(5 * d + 4, 16) + nl * layer + nl * (8 * d * d + 15 * d)
            if mixed:
                total += phi + (d * (2 * d + P + 2) + d + d * d + d) + rup(d * d + d, 4) + 5 * d * d + 12 * d
            assert flat.numel() == total == lib.psignn_weights_size(int(mixed), nl), (d, mixed, nl)
            assert eng.width_of(sd) == d
            # raw blocks sit where WLayout puts them
            F = "deqdss.f."
            assert torch.equal(flat[0:d], sd[F + "laynorm.weight"]) and torch.equal(flat[d:2 * d], sd[F + "laynorm.bias"])
            assert torch.equal(flat[2 * d:2 * d + 3 * d + P], sd[F + "alpha.0.weight"].reshape(-1))
            s0 = rup(5 * d + 4, 16)
            assert torch.equal(flat[s0:s0 + d * (2 * d + 3)], sd[F + "phi_to_list.0.mlp.mlp.0.weight"].reshape(-1))
            t0 = total - nl * (8 * d * d + 15 * d) - (5 * d * d + 12 * d if mixed else 0)
            assert torch.equal(flat[t0:t0 + d * d].reshape(d, d), sd[F + "phi_to_list.0.mlp.mlp.0.weight"][:, d:2 * d].t())
    # a buffer packed for one width is not the length another library expects
    assert nat.lib(8).psignn_weights_size(0, 1) != nat.lib(16).psignn_weights_size(0, 1) != nat.lib().psignn_weights_size(0, 1)


def test_each_library_knows_its_width():
    nat, eng = pkg("_native"), pkg("engine")
    assert eng.D == 10 and eng.SUPPORTED_WIDTHS == (8, 10, 16) and nat.SIGNATURES["psignn_latent_dim"][1] == []
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "psignn_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+psignn_latent_dim\s*\(\s*void\s*\)\s*;", hdr)
    assert re.search(r"#ifndef PSIGNN_D\s*\n#define PSIGNN_D 10", hdr)
    assert nat.lib() is nat.lib(10) and nat.lib().psignn_latent_dim() == 10 and nat.lib_path(10) == nat.LIB_PATH
    assert ctypes.CDLL(nat.LIB_PATH).psignn_latent_dim() == 10
    forward = ("psignn_plan_create", "psignn_weights_size", "psignn_f_forward", "psignn_f_forward_p", "psignn_picard_p", "psignn_phi",
               "psignn_mlp2", "psignn_residual", "psignn_broyden_create_opts", "psignn_broyden_solve", "psignn_broyden_solve_batch",
               "psignn_broyden_ext_update", "psignn_fpiter_create", "psignn_anderson_update", "psignn_reload_knobs",
               "psignn_prof_enable", "psignn_prof_collect")
    derivative = ("psignn_f_jvp", "psignn_f_jvp_p", "psignn_f_vjp", "psignn_f_vjp_p", "psignn_lin_create", "psignn_f_param_vjp",
                  "psignn_f_vjp_backward", "psignn_broyden_solve_adjoint", "psignn_broyden_solve_adjoint_lin_batch",
                  "psignn_dsgps_forward", "psignn_dss_forward", "psignn_gmres_create")
    for w in WIDTHS:
        lib = nat.lib(w)
        assert lib is nat.lib(w) and lib is not nat.lib() and lib.psignn_latent_dim() == w and lib.width == w
        raw = ctypes.CDLL(nat.lib_path(w))
        assert os.path.basename(nat.lib_path(w)) == f"libpsignn_hip_d{w}.so"
        for name in forward:
            assert hasattr(raw, name), (w, name)
        for name in derivative:      # compiled out there; the binding turns the name into the refusal, before any call
            assert not hasattr(raw, name), (w, name)
            with pytest.raises(nat.NativeError, match=f"latent_dim {w} has forward inference only"):
                getattr(lib, name)()
        # every psignn_* entry a width library exports is declared in the header and bound (no private surface)
        import subprocess
        syms = subprocess.run(["nm", "-D", "--defined-only", nat.lib_path(w)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" T (psignn_[a-z0-9_]+)$", syms, flags=re.M))
        assert set(forward) <= exported <= set(nat.SIGNATURES), sorted(exported - set(nat.SIGNATURES))
        assert lib.psignn_version() == nat.lib().psignn_version()


@pytest.mark.parametrize("w", [0, 7, 12, 18, 10.5, "16"])
def test_unsupported_widths_name_the_supported_ones(w):
    nat, eng = pkg("_native"), pkg("engine")
    for make in (lambda: pkg("model_psignn").ModelPSIGNN(dict(latent_dim=w, n_layers=1)),
                 lambda: pkg("mixed").ModelDEQDSS(dict(latent_dim=w, n_layers=1)),
                 lambda: nat.lib(w),
                 lambda: eng.DeviceBroyden(n_elems=64, seq_len=4, threshold=3, width=w)):
        with pytest.raises(nat.NativeError, match=r"\(8, 10, 16\)"):
            make()
    if isinstance(w, int) and w > 0:
        sd = {"deqdss.f.laynorm.weight": torch.ones(w)}
        with pytest.raises(nat.NativeError, match=r"\(8, 10, 16\)"):
            eng.pack_weights(sd)


@pytest.mark.parametrize("d", WIDTHS)
def test_baselines_and_training_are_refused_before_any_native_call(d, monkeypatch):
    nat = pkg("_native")
    monkeypatch.setattr(nat, "lib", lambda *a: (_ for _ in ()).throw(AssertionError("the library was touched")))
    with pytest.raises(nat.NativeError, match=f"latent_dim {d} has forward inference only"):
        pkg("dsgps").ModelDSGPS(dict(latent_dim=d, k=3))
    with pytest.raises(nat.NativeError, match=f"latent_dim {d} has forward inference only"):
        pkg("dss").DeepStatisticalSolver(dict(latent_dim=d, k=3, alpha=1e-3, gamma=0.9))
    net = pkg("model_psignn").ModelDEQDSS(dict(latent_dim=d, n_layers=1))
    for mode in (net.train(), net.eval()):
        with pytest.raises(nat.NativeError, match=f"latent_dim {d} has forward inference only"):
            mode(object())      # decided on the host: the batch is never looked at
    deq = net.deqdss
    for call in (lambda: deq.train_forward(torch.zeros(3, d), object()),
                 lambda: deq.implicit_backward(None, None, object(), torch.zeros(3, d)),
                 lambda: deq.jac_loss_estimate(None, None, object()),
                 lambda: deq.power_method(None, None, object())):
        with pytest.raises(nat.NativeError, match="forward inference only"):
            call()
