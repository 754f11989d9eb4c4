"""tcs_mi355.train_ops' gate stages on the host side (no GPU): the four C ABI entry points, their bindings and their argument checks
(which come before any HIP call), the surface's validation, the cell patch on stub classes, and a restatement of the two ops from the
issue's formulas (any float dtype, any device) that, composed into the three cells in float64, reproduces the reference's own float32
values and gradients (tests/golden/train_gates.npz, tools/make_goldens_train_gates.py).  The difference is e_ref, the reference's
float32 error, which test_gpu_train_gates.py uses as the yardstick for the HIP kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN

NEW_SYMBOLS = ("tcs_gru_reset", "tcs_gru_reset_backward", "tcs_gru_update", "tcs_gru_update_backward")
CELLS = ("gru", "fuse", "hu")
KEEPS = {"gru": False, "fuse": True, "hu": True}           # z_keeps_h of each cell
EPS32 = 2.0 ** -24


def golden():
    return dict(np.load(os.path.join(GOLDEN, "train_gates.npz")))


def input_keys(cell):
    return ("zr", "q0", "wq", "h", "g") + (("cz", "cr", "cq") if cell == "gru" else ())


def grad_keys(cell):
    return ("dzr", "dq0", "dh") + (("dcz", "dcr", "dcq") if cell == "gru" else ())


def case_tensors(gold, cell, i, dtype=torch.float32, device="cpu"):
    return {k: torch.from_numpy(gold[f"{cell}_c{i}_{k}"]).to(device=device, dtype=dtype) for k in input_keys(cell)}


def reset_restate(r_pre, h, cr=None):
    return torch.sigmoid(r_pre if cr is None else r_pre + cr) * h


def update_restate(z_pre, q_pre, h, cz=None, cq=None, *, z_keeps_h):
    z = torch.sigmoid(z_pre if cz is None else z_pre + cz)
    q = torch.tanh(q_pre if cq is None else q_pre + cq)
    return z * h + (1 - z) * q if z_keeps_h else (1 - z) * h + z * q


def run_cell(cell, t, reset, update):
    """One cell of the golden file on the tensors of `t` (case_tensors) with the given two ops: zr is chunked as the reference does,
    the stand-in for convq is rh * wq + q0.  -> h_new and the gradients the golden file holds, in the dtype of `t`."""
    names = [k for k in input_keys(cell) if k not in ("g", "wq")]
    L = {k: t[k].clone().requires_grad_(True) for k in names}
    z_pre, r_pre = L["zr"].chunk(2, dim=1)
    rh = reset(r_pre, L["h"], L.get("cr"))
    h_new = update(z_pre, rh * t["wq"] + L["q0"], L["h"], L.get("cz"), L.get("cq"), z_keeps_h=KEEPS[cell])
    grads = torch.autograd.grad(h_new, [L[k] for k in names], t["g"])
    return {"h_new": h_new.detach(), **{"d" + k: g for k, g in zip(names, grads)}}


def restate(cell, t):
    return run_cell(cell, t, reset_restate, update_restate)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_bound_exported_and_abi_18():
    from tcs_mi355 import build, native
    build.build(verbose=False)
    assert "tcs_gates.hip" in build.SOURCES
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "tcs_mi355.h")).read()
    L = native.lib()
    for name in NEW_SYMBOLS:
        m = re.search(r"\b" + name + r"\(([^;]*?)\);", header, re.S)
        assert m, name
        assert name in native.SIGNATURES, name
        assert len(native.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
        assert hasattr(L, name), name
    assert L.tcs_abi_version() >= 18
    assert "18:" in header[:header.index("tcs_error_string")]


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    """A null required pointer, a batch stride below C*H*W, a non-positive size and a backward with no wanted output are
    TCS_EINVAL (-1).  The pointers are host memory: a call that got past the checks would not return an error code."""
    from tcs_mi355 import native
    L = native.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    B, C, H, W = 2, 2, 2, 3
    n = C * H * W
    # null required pointers
    assert L.tcs_gru_reset(None, n, p, n, None, 0, B, C, H, W, p, None) == -1
    assert L.tcs_gru_reset(p, n, None, n, None, 0, B, C, H, W, p, None) == -1
    assert L.tcs_gru_reset(p, n, p, n, None, 0, B, C, H, W, None, None) == -1
    assert L.tcs_gru_reset_backward(p, n, p, n, None, 0, None, B, C, H, W, p, p, None) == -1
    assert L.tcs_gru_reset_backward(p, n, None, n, None, 0, p, B, C, H, W, p, None, None) == -1       # grad_r_pre needs h
    assert L.tcs_gru_update(None, n, p, n, p, n, None, 0, None, 0, 0, B, C, H, W, p, None) == -1
    assert L.tcs_gru_update(p, n, None, n, p, n, None, 0, None, 0, 1, B, C, H, W, p, None) == -1
    assert L.tcs_gru_update(p, n, p, n, None, n, None, 0, None, 0, 0, B, C, H, W, p, None) == -1
    assert L.tcs_gru_update(p, n, p, n, p, n, None, 0, None, 0, 1, B, C, H, W, None, None) == -1
    assert L.tcs_gru_update_backward(None, n, p, n, p, n, None, 0, None, 0, p, 0, B, C, H, W, p, p, p, None) == -1
    assert L.tcs_gru_update_backward(p, n, p, n, p, n, None, 0, None, 0, None, 0, B, C, H, W, p, p, p, None) == -1
    assert L.tcs_gru_update_backward(p, n, None, n, p, n, None, 0, None, 0, p, 1, B, C, H, W, None, p, None, None) == -1   # grad_q_pre needs q_pre
    assert L.tcs_gru_update_backward(p, n, p, n, None, n, None, 0, None, 0, p, 1, B, C, H, W, p, None, None, None) == -1   # grad_z_pre needs h
    # no wanted gradient
    assert L.tcs_gru_reset_backward(p, n, p, n, None, 0, p, B, C, H, W, None, None, None) == -1
    assert L.tcs_gru_update_backward(p, n, p, n, p, n, None, 0, None, 0, p, 0, B, C, H, W, None, None, None, None) == -1
    # a batch stride below C*H*W, of an input and of a context term
    assert L.tcs_gru_reset(p, n - 1, p, n, None, 0, B, C, H, W, p, None) == -1
    assert L.tcs_gru_reset(p, n, p, n, p, n - 1, B, C, H, W, p, None) == -1
    assert L.tcs_gru_reset_backward(p, n, p, 0, None, 0, p, B, C, H, W, p, p, None) == -1
    assert L.tcs_gru_update(p, n, p, n - 1, p, n, None, 0, None, 0, 0, B, C, H, W, p, None) == -1
    assert L.tcs_gru_update(p, n, p, n, p, n, p, 1, None, 0, 0, B, C, H, W, p, None) == -1
    assert L.tcs_gru_update_backward(p, n, p, n, p, n, None, 0, p, -n, p, 0, B, C, H, W, p, p, p, None) == -1
    # non-positive sizes
    for dims in ((0, C, H, W), (B, 0, H, W), (B, C, -1, W), (B, C, H, 0)):
        assert L.tcs_gru_reset(p, n, p, n, None, 0, *dims, p, None) == -1
        assert L.tcs_gru_reset_backward(p, n, p, n, None, 0, p, *dims, p, p, None) == -1
        assert L.tcs_gru_update(p, n, p, n, p, n, None, 0, None, 0, 0, *dims, p, None) == -1
        assert L.tcs_gru_update_backward(p, n, p, n, p, n, None, 0, None, 0, p, 0, *dims, p, p, p, None) == -1


def test_golden_cases_cover_the_issue():
    gold = golden()
    cases = [tuple(int(v) for v in c) for c in gold["cases"]]
    assert [c[1:] for c in cases] == [(1, 3, 5, 7, 2), (2, 5, 6, 11, 2), (1, 1, 1, 1, 2), (1, 4, 4, 8, 2), (2, 3, 5, 7, 30)]
    assert os.path.getsize(os.path.join(GOLDEN, "train_gates.npz")) < 512 * 1024
    for cell in CELLS:
        for i, (_, B, C, H, W, spread) in enumerate(cases):
            t = case_tensors(gold, cell, i)
            assert t["zr"].shape == (B, 2 * C, H, W) and all(t[k].shape == (B, C, H, W) for k in input_keys(cell) if k != "zr")
            assert float(t["h"].abs().max()) < 1
            if spread >= 30:                              # some gate does saturate: float32 rounds it to exactly 0 or 1
                z = torch.sigmoid(t["zr"])
                assert bool(((z == 0) | (z == 1)).any())


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("i", range(5))
def test_restatement_reproduces_the_reference(cell, i):
    """The float64 restatement against the reference's float32 values and gradients.  Every stored number is a short chain (about a
    dozen) of float32 operations.  Its factors are gate quantities of magnitude <= 1 (|q - h| < 2) whose ABSOLUTE error is a few
    eps32 = 2^-24 (1 - z and 1 - q^2 cancel, so not relative to the factor), and each is at most 1-Lipschitz in the pre-activation it
    reads, whose own rounding is eps32 * |pre|.  The factors multiply 1 for h_new, and the upstream gradient, once directly and once
    through r * h and wq, for a gradient: 16 eps32 * max(1, largest |pre-activation|) * unit covers the chain, with unit = 1 for
    h_new and max|g| (1 + max|wq|) for a gradient.  Prints e_ref per tensor."""
    gold = golden()
    t64 = case_tensors(gold, cell, i, torch.float64)
    r64 = restate(cell, t64)
    pre = max(float(t64["zr"].abs().max()), float((t64["q0"].abs() + t64["wq"].abs()).max())) + 3 * (cell == "gru")
    for key in ("h_new",) + grad_keys(cell):
        ref = torch.from_numpy(gold[f"{cell}_c{i}_{key}"]).double()
        x64 = r64[key]
        assert ref.shape == x64.shape and bool(torch.isfinite(ref).all()), key
        scale, err = float(x64.abs().max()), float((ref - x64).abs().max())
        unit = 1.0 if key == "h_new" else float(t64["g"].abs().max()) * (1 + float(t64["wq"].abs().max()))
        tol = 16 * EPS32 * max(1.0, pre) * unit
        print(f"{cell}_c{i}_{key}: max {scale:.3e}  e_ref {err:.3e}  tol {tol:.3e}")
        assert scale > 0 and err <= tol, (key, err, tol)


def test_restatement_follows_the_issues_gradient_formulas():
    """The closed forms of the issue, in float64, against autograd through the restatement: both conventions."""
    g = torch.Generator().manual_seed(3)
    z_pre, q_pre, h, cz, cq, up = (torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64) for _ in range(6))
    r_pre, cr = z_pre, cz
    L = [x.clone().requires_grad_(True) for x in (r_pre, h, cr)]
    d_pre, d_h, d_c = torch.autograd.grad(reset_restate(*L), L, up)
    r = torch.sigmoid(r_pre + cr)
    assert torch.allclose(d_pre, up * h * r * (1 - r), atol=1e-14) and torch.equal(d_pre, d_c) and torch.allclose(d_h, up * r, atol=1e-14)
    z, q = torch.sigmoid(z_pre + cz), torch.tanh(q_pre + cq)
    for keep in (False, True):
        L = [x.clone().requires_grad_(True) for x in (z_pre, q_pre, h, cz, cq)]
        d_z, d_q, d_h, d_cz, d_cq = torch.autograd.grad(update_restate(*L, z_keeps_h=keep), L, up)
        wq, sign = ((1 - z), -1.0) if keep else (z, 1.0)
        assert torch.allclose(d_q, up * wq * (1 - q * q), atol=1e-14) and torch.allclose(d_h, up * (1 - wq), atol=1e-14)
        assert torch.allclose(d_z, sign * up * (q - h) * z * (1 - z), atol=1e-14)
        assert torch.allclose(d_cz, d_z, atol=1e-15) and torch.allclose(d_cq, d_q, atol=1e-15)


def test_validation():
    from tcs_mi355 import ops, train_ops as to
    a = torch.zeros(2, 3, 4, 5)
    with pytest.raises(TypeError):
        to.gru_update(a, a, a)                                              # z_keeps_h has no default
    with pytest.raises(TypeError):
        to.gru_update(a, a, a, None, None, True)                            # and is keyword-only
    with pytest.raises(ValueError):
        to.gru_reset(a, torch.zeros(2, 3, 4, 6))
    with pytest.raises(ValueError):
        to.gru_reset(a, a, torch.zeros(2, 1, 4, 5))
    with pytest.raises(ValueError):
        to.gru_reset(a.clone().requires_grad_(True), torch.zeros(1, 3, 4, 5))
    with pytest.raises(ValueError):
        to.gru_reset(torch.zeros(3, 4, 5), torch.zeros(3, 4, 5))
    with pytest.raises(ValueError):
        to.gru_update(a, torch.zeros(2, 6, 4, 5), a, z_keeps_h=False)
    with pytest.raises(ValueError):
        to.gru_update(a, a, a, cq=torch.zeros(2, 3, 5, 4), z_keeps_h=True)
    with pytest.raises(ValueError):
        to.gru_update(a.clone().requires_grad_(True), a, a, torch.zeros(2, 3, 4, 4), z_keeps_h=True)
    # CPU tensors: refused like every other wrapper, with and without grad
    for x in (a, a.clone().requires_grad_(True)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            to.gru_reset(x, a)
        with pytest.raises(RuntimeError, match="no CPU path"):
            to.gru_update(x, a, a, z_keeps_h=False)
    # the layouts read in place: chunk / split views along dim 1, a padded batch stride; not a transposed or a strided plane
    wide = torch.zeros(2, 6, 4, 5)
    assert all(ops.gate_view_ok(v) for v in wide.chunk(2, 1)) and all(ops.gate_view_ok(v) for v in wide.split(2, 1))
    assert ops.gate_view_ok(torch.zeros(2, 70)[:, :60].view(2, 3, 4, 5)) and ops.gate_view_ok(wide[:1])
    assert not ops.gate_view_ok(a.transpose(2, 3)) and not ops.gate_view_ok(wide[:, ::2]) and not ops.gate_view_ok(wide[..., ::2])
    assert not ops.gate_view_ok(a[:1].expand(2, 3, 4, 5))                   # batch stride 0 < C*H*W


def test_the_backward_path_never_reads_the_device_on_the_host():
    import inspect

    from tcs_mi355 import ops, train_ops
    src = "".join(inspect.getsource(f) for f in (train_ops._GruReset.backward, train_ops._GruUpdate.backward, ops.gate_reset_backward,
                                                 ops.gate_update_backward, ops._gate_in, ops._gate_grad, ops._gate_dims, ops.gate_view_ok))
    for word in (".item(", ".cpu(", ".tolist(", "synchronize", ".numpy(", "zeros"):
        assert word not in src, word


def test_patch_reference_cells_and_undo():
    """The patch swaps the three forwards of the classes it is given and the returned function restores them."""
    from types import SimpleNamespace

    from tcs_mi355 import train_ops as to

    def stub():
        class Cell:
            def forward(self, *a, **k):
                return "original"
        return Cell
    ConvGRU, Lightfuse, Updater = stub(), stub(), stub()
    mod = SimpleNamespace(ConvGRU=ConvGRU, Lightfuse=Lightfuse, HiddenstateUpdater=Updater)
    originals = (ConvGRU.forward, Lightfuse.forward, Updater.forward)
    undo = to.patch_reference_cells(mod)
    for cls in (ConvGRU, Lightfuse, Updater):
        assert cls.forward.__module__ == to.__name__
    assert len({ConvGRU.forward, Lightfuse.forward, Updater.forward}) == 3
    undo()
    assert (ConvGRU.forward, Lightfuse.forward, Updater.forward) == originals
    assert ConvGRU().forward() == "original" and Lightfuse().forward() == "original" and Updater().forward() == "original"
