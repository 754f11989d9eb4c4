"""tcs_mi355.train_ops on the host side (no GPU): the new C ABI entry points and their bindings, the surface's validation, and an
autograd restatement of the two ops written from SURVEY.md A6 / A7 (any float dtype, any device) that, in float64, reproduces the
reference's own float32 outputs and gradients (tests/golden/train_ops.npz, tools/make_goldens_train_ops.py).  The difference is
e_ref, the reference's float32 error, which test_gpu_train_ops.py uses as the yardstick for the HIP backward."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

NEW_SYMBOLS = ("tcs_upsample_flow", "tcs_upsample_flow_pair", "tcs_convex_upsample_backward_workspace_floats",
               "tcs_convex_upsample_backward", "tcs_convex_upsample_pair_backward", "tcs_refine_blend", "tcs_refine_blend_backward")
UP_GRADS = ("dflow_a", "dflow_b", "dmask")
BLEND_GRADS = ("dlogits", "ddisp_grads")


def golden():
    return dict(np.load(os.path.join(GOLDEN, "train_ops.npz")))


def case_tensors(gold, i, dtype=torch.float32, device="cpu"):
    keys = ("flow_a", "flow_b", "mask", "g_a", "g_b", "logits", "disp_grads", "disp", "g_r")
    return {k: torch.from_numpy(gold[f"c{i}_{k}"]).to(device=device, dtype=dtype) for k in keys}


def neighbours(x, mode):
    """[N,C,H,W] -> [N,C,9,H,W]: plane k = 3v+u holds x at (y+v-1, x+u-1), zero- or replicate-padded."""
    H, W = x.shape[-2:]
    xp = F.pad(x, (1, 1, 1, 1), mode=mode)
    return torch.stack([xp[..., v:v + H, u:u + W] for v in range(3) for u in range(3)], dim=2)


def upsample_restate(flow, mask):
    """up[n,0,4h+i,4w+j] = sum_k softmax_k(mask[n, k*16+4i+j, h, w]) * 4 flow_pad0[n, 0, h+k//3-1, w+k%3-1]."""
    N, _, H, W = flow.shape
    s = torch.softmax(mask.view(N, 9, 16, H, W), dim=1)
    up = (s * neighbours(4 * flow, "constant")[:, 0, :, None]).sum(1)                    # [N,16,H,W], channel i*4 + j
    return up.view(N, 4, 4, H, W).permute(0, 3, 1, 4, 2).reshape(N, 1, 4 * H, 4 * W)


def blend_restate(logits, disp_grads, disp):
    """cand_k = d_n + gx_n (1-u) + gy_n (1-v), d replicate-padded, gradient zero-padded; refined = sum_k softmax_k cand_k."""
    d = neighbours(disp, "replicate")[:, 0]
    g = neighbours(disp_grads, "constant")
    cu = torch.tensor([1 - (k % 3) for k in range(9)], dtype=logits.dtype, device=logits.device).view(1, 9, 1, 1)
    cv = torch.tensor([1 - (k // 3) for k in range(9)], dtype=logits.dtype, device=logits.device).view(1, 9, 1, 1)
    cand = d + g[:, 0] * cu + g[:, 1] * cv
    return (torch.softmax(logits, dim=1) * cand).sum(1, keepdim=True)


def restate(t):
    """Outputs and gradients of both ops on the tensors of `t` (case_tensors), in their dtype, with the pair's semantics: flow_a's
    output reads the mask detached."""
    fa, fb, mask, logits, grads = (t[k].clone().requires_grad_(True) for k in ("flow_a", "flow_b", "mask", "logits", "disp_grads"))
    up_a, up_b = upsample_restate(fa, mask.detach()), upsample_restate(fb, mask)
    dfa, dfb, dm = torch.autograd.grad((up_a * t["g_a"]).sum() + (up_b * t["g_b"]).sum(), [fa, fb, mask])
    refined = blend_restate(logits, grads, t["disp"])
    dl, dg = torch.autograd.grad((refined * t["g_r"]).sum(), [logits, grads])
    return {"up_a": up_a.detach(), "up_b": up_b.detach(), "dflow_a": dfa, "dflow_b": dfb, "dmask": dm, "refined": refined.detach(),
            "dlogits": dl, "ddisp_grads": dg}


def softmax_ties(x, dim):
    top = torch.topk(x, 2, dim=dim).values
    return int((top.select(dim, 0) == top.select(dim, 1)).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_bound_exported_and_abi_16():
    from tcs_mi355 import build, native
    build.build(verbose=False)
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "tcs_mi355.h")).read()
    L = native.lib()
    for name in NEW_SYMBOLS:
        m = re.search(r"\b" + name + r"\(([^;]*?)\);", header, re.S)
        assert m, name
        assert name in native.SIGNATURES, name
        assert len(native.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
        assert hasattr(L, name), name
    assert L.tcs_abi_version() >= 16
    assert "16:" in header[:header.index("tcs_error_string")]


def test_entry_points_reject_bad_arguments_before_launch():
    from tcs_mi355 import native
    L = native.lib()
    assert L.tcs_upsample_flow(None, None, 1, 4, 4, None, None) == -1
    assert L.tcs_upsample_flow_pair(None, None, None, 1, 4, 4, None, None, None) == -1
    assert L.tcs_convex_upsample_backward(None, None, None, 1, 4, 4, None, None, None, None) == -1
    assert L.tcs_convex_upsample_pair_backward(None, None, None, None, 1, 4, 4, None, None, None, None, None) == -1
    assert L.tcs_refine_blend(None, None, None, 1, 4, 4, None, None) == -1
    assert L.tcs_refine_blend_backward(None, None, None, None, 1, 4, 4, None, None, None) == -1
    assert L.tcs_convex_upsample_backward_workspace_floats(2, 5, 7, 2) == 2 * 9 * 2 * 5 * 7
    assert L.tcs_convex_upsample_backward_workspace_floats(2, 5, 7, 0) == 0


def test_train_ops_imports_without_core():
    code = ("import sys; import tcs_mi355.train_ops as t; assert not any(m == 'core' or m.startswith('core.') for m in sys.modules); "
            "assert all(hasattr(t, n) for n in ('upsample_flow', 'upsample_flow_pair', 'refine_blend', 'patch_reference'))")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    subprocess.run([sys.executable, "-c", code], check=True, env=env)


def test_golden_cases_cover_the_issue():
    gold = golden()
    cases = [tuple(int(v) for v in c) for c in gold["cases"]]
    assert {c[1] for c in cases} == {1, 2}
    assert any(c[2] == 1 for c in cases) and any(c[3] == 1 for c in cases) and any(c[4] >= 30 for c in cases)
    assert any(c[2] % 4 and c[3] % 4 for c in cases)
    assert os.path.getsize(os.path.join(GOLDEN, "train_ops.npz")) < 1024 * 1024
    for i, (_, B, H, W, spread) in enumerate(cases):
        t = case_tensors(gold, i)
        assert t["mask"].shape == (B, 144, H, W) and t["logits"].shape == (B, 9, H, W) and t["g_a"].shape == (B, 1, 4 * H, 4 * W)
        # no exact tie between the two largest logits of any softmax: the reference's max() backward stays out of the comparison
        assert softmax_ties(t["mask"].view(B, 9, 16, H, W), 1) == 0 and softmax_ties(t["logits"], 1) == 0, i
        if spread >= 30:                                  # the softmax does saturate: some winner holds all but 1e-6 of the weight
            assert float(torch.softmax(t["logits"], 1).max()) > 1 - 1e-6


@pytest.mark.parametrize("i", range(5))
def test_restatement_reproduces_the_reference(i):
    """float64 restatement against the reference's float32 outputs and gradients: to 1e-5 of each tensor's largest magnitude (a few
    float32 roundings of sums of <= 144 terms).  Prints e_ref per tensor."""
    gold = golden()
    r64 = restate(case_tensors(gold, i, torch.float64))
    for key, x64 in r64.items():
        ref = torch.from_numpy(gold[f"c{i}_{key}"]).double()
        assert ref.shape == x64.shape and bool(torch.isfinite(ref).all()), key
        scale, err = float(x64.abs().max()), float((ref - x64).abs().max())
        print(f"c{i}_{key}: max {scale:.3e}  e_ref {err:.3e}  ({err / scale:.2e} of max)")
        assert scale > 0 and err <= 1e-5 * scale, (key, err, scale)


def test_validation():
    from tcs_mi355 import train_ops as to
    f, m = torch.zeros(1, 1, 4, 6), torch.zeros(1, 144, 4, 6)
    with pytest.raises(ValueError):
        to.upsample_flow(torch.zeros(1, 2, 4, 6), m)                       # D != 1
    with pytest.raises(ValueError):
        to.upsample_flow(f, torch.zeros(1, 576, 4, 6))                     # factor 8
    with pytest.raises(ValueError):
        to.upsample_flow_pair(f, torch.zeros(1, 1, 4, 5), m)
    with pytest.raises(ValueError):
        to.upsample_flow_pair(f.clone().requires_grad_(True), f, torch.zeros(1, 144, 5, 6))
    lg, g, d = torch.zeros(1, 9, 4, 6), torch.zeros(1, 2, 4, 6), torch.zeros(1, 1, 4, 6)
    with pytest.raises(ValueError):
        to.refine_blend(torch.zeros(1, 8, 4, 6), g, d)
    with pytest.raises(ValueError):
        to.refine_blend(lg.clone().requires_grad_(True), torch.zeros(1, 1, 4, 6), d)
    with pytest.raises(NotImplementedError):
        to.refine_blend(lg, g, d.clone().requires_grad_(True))
    # CPU tensors: refused like every other wrapper, with and without grad
    for args in ((f, m), (f.clone().requires_grad_(True), m)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            to.upsample_flow(*args)
    with pytest.raises(RuntimeError, match="no CPU path"):
        to.upsample_flow_pair(f, f, m.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="no CPU path"):
        to.refine_blend(lg.clone().requires_grad_(True), g, d)
    with pytest.raises(RuntimeError, match="no CPU path"):
        to.refine_blend(lg, g, d)


def test_the_backward_path_never_reads_the_device_on_the_host():
    from tcs_mi355 import ops, train_ops
    src = "".join(inspect.getsource(f) for f in (
        train_ops._Upsample.backward, train_ops._UpsamplePair.backward, train_ops._RefineBlend.backward, ops.convex_upsample_backward,
        ops.convex_upsample_pair_backward, ops.refine_blend_backward, ops._grad16))
    for word in (".item(", ".cpu(", ".tolist(", "synchronize", ".numpy(", "zeros"):
        assert word not in src, word


def test_patch_reference_and_undo():
    """The patch swaps the two methods of the classes it is given and the returned function restores them."""
    from types import SimpleNamespace

    from tcs_mi355 import train_ops as to

    class TCStereo:
        def upsample_flow(self, flow, mask, scale=True):
            return "original"

    class DispRefine:
        def forward(self, *a, **k):
            return "original"
    tc, up = SimpleNamespace(TCStereo=TCStereo), SimpleNamespace(DispRefine=DispRefine)
    undo = to.patch_reference(tc, up)
    assert TCStereo.upsample_flow.__module__ == to.__name__ and DispRefine.forward.__module__ == to.__name__
    m = TCStereo()
    m.args = SimpleNamespace(n_downsample=2)
    assert m.upsample_flow(torch.zeros(1, 1, 2, 2), torch.zeros(1, 144, 2, 2), scale=False) == "original"
    assert m.upsample_flow(torch.zeros(1, 2, 2, 2), torch.zeros(1, 144, 2, 2)) == "original"
    undo()
    assert TCStereo().upsample_flow(None, None) == "original" and DispRefine().forward() == "original"
