"""CPU checks for the correlation block's gradients: the oracle's correlation functions, differentiated by
torch autograd in fp64, against the reference's own autograd (tests/golden/corr_grad.npz); the C ABI 14 entry points; and that
`tcs_mi355.corr` imports without any `core` package.  Shared helpers for tests/test_gpu_corr_grad.py live here."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT

NEW_SYMBOLS = ("tcs_corr_lookup_backward", "tcs_corr_build_backward", "tcs_corr_build_backward_scratch_bytes")


def golden():
    return dict(np.load(os.path.join(GOLDEN, "corr_grad.npz")))


def golden_case(g):
    from tcs_mi355 import synth
    seed, B, C, H, W, r = (int(v) for v in g["case"])
    return synth.make_corr_grad_case(seed, B, C, H, W, r), r


def digest(case):
    import hashlib
    h = hashlib.sha256()
    for k in sorted(case):
        h.update(np.ascontiguousarray(case[k]).tobytes())
    return h.hexdigest()[:16]


def _leaves(case, dtype, device, lookups):
    f1 = torch.from_numpy(case["fmap1"]).to(device=device, dtype=dtype).requires_grad_(True)
    f2 = torch.from_numpy(case["fmap2"]).to(device=device, dtype=dtype).requires_grad_(True)
    coords = [torch.from_numpy(case["coords"][k]).to(device=device, dtype=dtype).requires_grad_(True) for k in range(lookups)]
    return f1, f2, coords


def _score(case, outs, cost, main, device, dtype):
    loss = 0.0
    for k, o in enumerate(outs):
        loss = loss + (o * torch.from_numpy(case["g_lookup"][k]).to(device=device, dtype=dtype)).sum()
    if cost is not None:
        loss = loss + (cost * torch.from_numpy(case["g_cost"]).to(device=device, dtype=dtype)).sum()
    if main is not None:
        loss = loss + (main * torch.from_numpy(case["g_main"]).to(device=device, dtype=dtype)).sum()
    return loss


def oracle_grads(oracle, case, radius, lookups=None, cost=True, main=True):
    """(grad_fmap1, grad_fmap2, [grad_coords_k]) of the scored step: the oracle's functions under fp64 autograd on the CPU."""
    lookups = case["coords"].shape[0] if lookups is None else lookups
    f1, f2, coords = _leaves(case, torch.float64, "cpu", lookups)
    vol = oracle.corr_volume(f1, f2)
    pyr = oracle.corr_pyramid(vol)
    outs = [oracle.corr_lookup(pyr, c, radius) for c in coords]
    cv = oracle.masked_cost_volume(vol) if (cost or main) else None
    mc = oracle.argmax_disp(cv)[1] if main else None
    loss = _score(case, outs, cv if cost else None, mc, "cpu", torch.float64)
    g = torch.autograd.grad(loss, [f1, f2, *coords], allow_unused=True)
    g = [torch.zeros_like(t) if x is None else x for x, t in zip(g, [f1, f2, *coords])]
    return g[0], g[1], list(g[2:])


def torch_reference_block(f1, f2, radius):
    """The reference's formulation (corr.py:8-79, utils.py:82-97) restated in torch ops: F.normalize, einsum, avg_pool2d,
    grid_sample.  Returns (lookup(coords), cost_volume, main_cost)."""
    B, C, H, W = f1.shape
    n1, n2 = F.normalize(f1, dim=1), F.normalize(f2, dim=1)
    vol = torch.einsum('aijk,aijh->ajkh', n1, n2).reshape(B * H * W, 1, 1, W)
    pyr = [vol]
    for _ in range(3):
        pyr.append(F.avg_pool2d(pyr[-1], [1, 2], stride=[1, 2]))
    cost = vol.reshape(B, H, W, W).permute(0, 3, 1, 2)
    j = torch.arange(W, device=f1.device)
    cost = cost * (j.view(1, W, 1, 1) <= j.view(1, 1, 1, W)).to(cost.dtype)

    def lookup(coords):
        c = coords[:, :1].permute(0, 2, 3, 1).reshape(B * H * W, 1, 1, 1)
        dx = torch.linspace(-radius, radius, 2 * radius + 1, device=f1.device, dtype=f1.dtype).view(2 * radius + 1, 1)
        out = []
        for i, lv in enumerate(pyr):
            x = dx + c / 2 ** i
            Wi = lv.shape[-1]
            grid = torch.cat([2 * x / (Wi - 1) - 1, torch.zeros_like(x)], dim=-1)
            out.append(F.grid_sample(lv, grid, align_corners=True).view(B, H, W, -1))
        return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous()

    def main_cost():
        main, idx = cost.max(dim=1, keepdim=True)
        near = (j.view(1, W, 1, 1) >= idx - 1.5) & (j.view(1, W, 1, 1) < idx + 1.5)
        sub = torch.where(near, torch.zeros_like(cost), cost).max(dim=1, keepdim=True)[0]
        return main * (main - sub > 0.3).to(cost.dtype)

    return lookup, cost, main_cost


def torch_reference_grads(case, radius, device, lookups=None, cost=True, main=True, dtype=torch.float32):
    """The same scored step through torch_reference_block (the bar's fp32 reference on the same device)."""
    lookups = case["coords"].shape[0] if lookups is None else lookups
    f1, f2, coords = _leaves(case, dtype, device, lookups)
    lookup, cv, mc = torch_reference_block(f1, f2, radius)
    outs = [lookup(c) for c in coords]
    loss = _score(case, outs, cv if cost else None, mc() if main else None, device, dtype)
    g = torch.autograd.grad(loss, [f1, f2, *coords], allow_unused=True)
    g = [torch.zeros_like(t) if x is None else x for x, t in zip(g, [f1, f2, *coords])]
    return g[0], g[1], list(g[2:])


def eps_pixels(fmap):
    """[B,1,H,W] bool: pixels whose feature norm is below F.normalize's eps (their gradient is dn / eps)."""
    f = torch.as_tensor(fmap).double()
    return (f.norm(dim=1, keepdim=True) < 1e-12)


def grad_error_ok(got, f32, f64, groups=None):
    """The bar: |got - f64| <= 4 |f32 - f64| + 1e-7 max|f64|, each max taken over a group of elements (default: all).  The eps
    branch's pixels (gradients ~1e12 times larger) form a group of their own so that they do not swamp the floor of the rest."""
    got, f32, f64 = (torch.as_tensor(t).detach().cpu().double() for t in (got, f32, f64))
    if groups is None:
        groups = [torch.ones_like(f64, dtype=torch.bool)]
    msgs = []
    for m in groups:
        m = m.expand_as(f64).cpu()
        if not bool(m.any()):
            continue
        e = float((got - f64)[m].abs().max())
        e32 = float((f32 - f64)[m].abs().max())
        bar = 4 * e32 + 1e-7 * float(f64[m].abs().max())
        if not e <= bar:
            msgs.append(f"err {e:.3e} > bar {bar:.3e} (fp32 ref err {e32:.3e}, max|g| {float(f64[m].abs().max()):.3e})")
    return not msgs, "; ".join(msgs)


def fmap_groups(fmap):
    z = eps_pixels(fmap)
    return [~z, z]


# ---------------------------------------------------------------------------------------------------------------------------
def test_oracle_grads_match_reference_golden(oracle):
    g = golden()
    case, r = golden_case(g)
    assert digest(case) == str(g["digest"]), "synth.make_corr_grad_case no longer reproduces the golden's inputs"
    g1, g2, gc = oracle_grads(oracle, case, r)
    for got, ref, f in ((g1, g["grad_fmap1"], case["fmap1"]), (g2, g["grad_fmap2"], case["fmap2"])):
        for m in fmap_groups(f):
            m = m.expand(*ref.shape).numpy()
            scale = float(np.abs(ref[m]).max())
            assert np.abs(got.numpy()[m] - ref[m]).max() <= 2e-5 * scale, (np.abs(got.numpy()[m] - ref[m]).max(), scale)
    # At an integer coordinate the lerp has a kink: the floor-based derivative (the oracle, the kernels) is the right-hand one, and
    # grid_sample takes whichever side the fp32 rounding of its normalise / unnormalise round trip lands on, per tap and level.
    # There the golden pins only the extreme coordinates (gradient 0); tests/test_gpu_corr_grad.py checks the integer case
    # against the fp64 oracle.
    gc = np.stack([c.numpy() for c in gc])
    ref = g["grad_coords"]
    kink = (np.round(case["coords"]) == case["coords"]) & (np.abs(case["coords"]) < 1000)
    scale = float(np.abs(ref).max())
    assert np.abs(gc - ref)[~kink].max() <= 2e-5 * scale, np.abs(gc - ref)[~kink].max()
    assert (~kink[:2]).all() and (~kink[2]).sum() == 4


def test_golden_covers_the_cases():
    g = golden()
    case, r = golden_case(g)
    assert case["fmap1"].shape[1] == 256 and case["fmap1"].shape[3] % 8 != 0       # C=256, ragged W
    c = case["coords"]
    assert c.shape[0] == 3
    assert np.isin([1000.0, -1000.0, 3e9, -3e9], c).all()
    assert (np.round(c[2]) == c[2]).all()                                             # integer coords
    assert (c < -r).any() and (c > case["fmap1"].shape[3] + r).any()                   # taps out of range at both ends
    assert bool(eps_pixels(case["fmap1"]).any()) and bool(eps_pixels(case["fmap2"]).any())
    assert np.abs(g["grad_fmap1"]).max() > 0 and np.abs(g["grad_coords"]).max() > 0
    assert os.path.getsize(os.path.join(GOLDEN, "corr_grad.npz")) < 512 * 1024


def test_abi_14_declares_binds_and_exports_backward():
    from tcs_mi355 import native
    lib = native.lib()
    assert lib.tcs_abi_version() >= 14
    header = open(os.path.join(ROOT, "include", "tcs_mi355.h")).read()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header, name
        assert name in native.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.tcs_corr_build_backward_scratch_bytes(1, 256, 8, 16) == 0
    # argument checks run before any launch, so they are testable without a GPU
    assert lib.tcs_corr_lookup_backward(None, None, None, None, None, None, 1, 8, 16, 4, None, None, None) == -1
    assert lib.tcs_corr_build_backward(None, None, None, None, 1, 8, 8, 16, None, None, None, None) == -1


def test_ops_backward_wrappers_check_shapes():
    from tcs_mi355 import ops
    pyr = ops.CorrPyramid([torch.zeros(1)] * 4, 1, 4, 16, torch.zeros(1))
    with pytest.raises(ValueError, match="coords"):
        ops.corr_lookup_backward(pyr, torch.zeros(1, 1, 4, 15), torch.zeros(1, 36, 4, 16))
    with pytest.raises(ValueError, match="grad_out"):
        ops.corr_lookup_backward(pyr, torch.zeros(1, 1, 4, 16), torch.zeros(1, 35, 4, 16))
    with pytest.raises(ValueError, match="grad_vol"):
        ops.corr_build_backward(torch.zeros(1, 8, 4, 16), torch.zeros(1, 8, 4, 16), pyr, torch.zeros(1, 4, 16, 15))
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        ops.corr_lookup_backward(pyr, torch.zeros(1, 1, 4, 16), torch.zeros(1, 36, 4, 16))


def test_corr_module_imports_without_core(tmp_path):
    """The reference's training script has its own `core` on sys.path: tcs_mi355.corr must not import any `core`."""
    stand_in = tmp_path / "core"
    stand_in.mkdir()
    (stand_in / "__init__.py").write_text("raise ImportError('the stand-in core package was imported')\n")
    script = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {str(tmp_path)!r})
        sys.path.insert(1, {os.path.join(ROOT, "temporally-consistent-stereo-matching_amd")!r})
        import tcs_mi355.corr as c
        assert 'core' not in sys.modules, 'core was imported'
        assert c.CorrBlock1D.__module__ == 'tcs_mi355.corr'
        print('ok')
    """)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_core_corr_reexports_the_same_class():
    import core.corr
    import tcs_mi355.corr
    assert core.corr.CorrBlock1D is tcs_mi355.corr.CorrBlock1D


def test_grad_path_needs_the_device():
    """A CPU tensor that requires grad reaches the same loud no-CPU-path error as the inference path."""
    from tcs_mi355.corr import CorrBlock1D
    f = torch.zeros(1, 8, 4, 16, requires_grad=True)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        CorrBlock1D(f, f)
