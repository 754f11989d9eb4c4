"""The differentiable training objective on the host side (no GPU): the tcs_*loss*_bwd C ABI, tcs_mi355.train_losses' surface and
validation, and an fp64 autograd restatement of train_stereo.py:362-399 (the functions of test_losses_host.py: masks from the
reference's float32 ops, values in float64) against the reference's own float32 gradients (tests/golden/loss_grad.npz,
tools/make_goldens_loss_grad.py).  test_gpu_loss_grad.py holds the HIP backward to the same restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_losses_host as H
from conftest import GOLDEN

NEW_SYMBOLS = ("tcs_loss_finish_counts", "tcs_sequence_loss_bwd", "tcs_init_loss_bwd", "tcs_grad_normal_loss_bwd")
INPUTS = ("up", "q", "grad", "flow_mono", "flow_init", "cost_volume")
PART_INPUTS = {"seq": ("up", "flow_mono", "flow_init"), "init": ("cost_volume",), "norm": ("q",), "grad": ("grad",)}
HINGE_WINDOW = 1e-6


def golden():
    return dict(np.load(os.path.join(GOLDEN, "loss_grad.npz")))


def init_loss_torch(cv, flow, v, k, thres=0.5):
    """train_stereo.py:138-180 in plain torch ops in cv's dtype (masks from the float32 flow) -> (loss, internals)."""
    dtype = cv.dtype
    B, D, h, w = cv.shape
    fs = 0.25 * F.interpolate(flow, scale_factor=0.25, mode="nearest")
    vi = (F.interpolate(v.float(), scale_factor=0.25, mode="bilinear", align_corners=True) == 1) & (fs.abs() < 175)
    idx = torch.arange(w, device=cv.device).view(1, 1, 1, -1).to(dtype) + fs.to(dtype)
    mask = (idx >= 0) & (idx <= D - 1) & vi
    idx = idx.clamp(0, D - 1)
    df = idx.floor().long()
    fr = idx - df
    phi = fr * cv.gather(1, (df + 1).clamp(0, D - 1)) + (1 - fr) * cv.gather(1, df.clamp(0, D - 1))
    cand = torch.arange(D, device=cv.device).view(1, -1, 1, 1).to(dtype)
    excl = ((cand >= idx - 1.5) & (cand < idx + 1.5)) | ~mask
    filled = cv.masked_fill(excl, 0)
    top, top_i = torch.topk(filled, k=k, dim=1)
    hinge = top + thres - phi.detach()
    loss = (1 - phi[mask].mean()) + hinge.clamp(min=0)[mask.expand(-1, k, -1, -1)].mean()
    return loss, dict(mask=mask, excl=excl, filled=filled, top_i=top_i, hinge=hinge)


def objective_torch(L, flow, valid_raw, iters, k, dense, thres=0.5):
    """Lines 362-399 in plain torch ops on the tensors of L (`up`, `q`, `grad` stacked, `flow_mono`, `flow_init`, `cost_volume`; any
    float dtype and device), masks and targets from the reference's float32 ops -> ({'total', 'seq', 'init', 'norm', 'grad'}, internals).
    A mean over an empty mask is NaN with an all-zero gradient, as the reference's."""
    dtype, n = L["up"].dtype, iters
    gam = 0.9 ** (15 / (n - 1))
    wts = [gam ** (n - i - 1) for i in range(n)]
    v, g, gm, nrm, nm = H.targets(flow, valid_raw)
    gt = flow.to(dtype)

    def mean(x, m):
        return x[m].mean()
    seq = 0.1 * mean((L["flow_init"] - gt).abs(), v) + 0.1 * mean((L["flow_mono"] - gt).abs(), v)
    for i in range(n):
        seq = seq + wts[i] * mean((L["up"][i, 0] - gt).abs() + 1.2 * (L["up"][i, 1] - gt).abs(), v)
    ini, aux = init_loss_torch(L["cost_volume"], flow, v, k, thres)
    qv = H.quarter_valid(v, dense)
    gv, nv = qv & gm, qv & nm
    grad = sum(wts[i] * mean((L["grad"][i] - g.to(dtype)).abs().mean(1, keepdim=True), gv) for i in range(n))
    ng = nrm.to(dtype)

    def nl(f):
        p = H.normal_xy(-f)
        return 0.5 * (p - ng).abs().mean(1, keepdim=True) + 0.5 * (1 - (p * ng).sum(1, keepdim=True))
    norm = sum(wts[i] * (mean(nl(L["q"][i, 0]), nv) + 1.2 * mean(nl(L["q"][i, 1]), nv)) for i in range(n))
    losses = {"total": seq + ini + 0.25 * norm + 5 * grad, "seq": seq, "init": ini, "norm": norm, "grad": grad}
    return losses, dict(aux, v=v, g=g, gv=gv, nv=nv, ng=ng, gt=gt)


def restate_grads(case, iters, k, dense, thres=0.5, dtype=torch.float64):
    """Lines 362-399 under float64 autograd (dtype=torch.float32: the same ops in the reference's precision, for settings the golden
    file does not hold).  -> (grads, info): grads['total' | 'seq' | 'init' | 'norm' | 'grad'][input name] (a part alone: only what it
    reads); info: the masks, the kink maps (True = the element's input sits on a kink and may be left out of a comparison) and, for
    the cost volume, the number `active` of real top-k candidates with an active hinge."""
    t = {key: torch.from_numpy(v) for key, v in case.items()}
    L = {n: t[n].to(dtype).requires_grad_(True) for n in INPUTS}
    n = iters
    losses, x = objective_torch(L, t["flow"], t["valid"], iters, k, dense, thres)
    grads = {"total": dict(zip(INPUTS, torch.autograd.grad(losses["total"], [L[i] for i in INPUTS], retain_graph=True)))}
    for part in ("seq", "init", "norm", "grad"):
        wrt = PART_INPUTS[part]
        grads[part] = dict(zip(wrt, torch.autograd.grad(losses[part], [L[i] for i in wrt], retain_graph=True)))
    v, gv, nv, ng, gt, mask, excl, hinge = x["v"], x["gv"], x["nv"], x["ng"], x["gt"], x["mask"], x["excl"], x["hinge"]
    B, D, h, w = L["cost_volume"].shape
    with torch.no_grad():
        real = ~excl.gather(1, x["top_i"])                                     # a top-k slot held by a real entry
        srt = torch.sort(x["filled"], dim=1, descending=True).values
        tie = (srt[:, k - 1:k] == srt[:, k:k + 1]) & (srt[:, k - 1:k] != 0) if D > k else torch.zeros_like(mask)
        col_kink = mask & (((hinge.abs() < HINGE_WINDOW) & real).any(1, keepdim=True) | tie)
        q_kink = torch.zeros(n, 2, B, 1, h, w, dtype=torch.bool)
        # n_x is identically 0 in the last column and n_y in the last row (replicate pad): equal to the target there is no kink
        varies = torch.ones(1, 3, h, w, dtype=torch.bool)
        varies[:, 0, :, -1] = False
        varies[:, 1, -1, :] = False
        for i in range(n):
            for r in range(2):
                on = (H.normal_xy(-L["q"][i, r]) == ng) & varies
                on = on.any(1, keepdim=True) & nv
                q_kink[i, r] = on
                q_kink[i, r, :, :, :, 1:] |= on[:, :, :, :-1]
                q_kink[i, r, :, :, 1:, :] |= on[:, :, :-1, :]
        kinks = {"up": (L["up"] == gt) & v, "flow_mono": (L["flow_mono"] == gt) & v, "flow_init": (L["flow_init"] == gt) & v,
                 "grad": (L["grad"] == x["g"].to(dtype)) & gv, "q": q_kink, "cost_volume": col_kink.expand(-1, D, -1, -1)}
        active = ((hinge >= 0) & real).sum(1, keepdim=True)
    info = {"valid": v, "grad_valid": gv, "norm_valid": nv, "init_mask": mask, "kinks": kinks, "active": active,
            "count_init": int(mask.sum())}
    return grads, info


# ---------------------------------------------------------------------------------------------------------------------------------
def test_bwd_symbols_declared_bound_exported_and_abi_15():
    from tcs_mi355 import build, native
    build.build(verbose=False)
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "tcs_mi355.h")).read()
    L = native.lib()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header, name
        assert name in native.SIGNATURES, name
        assert hasattr(L, name), name
    assert L.tcs_abi_version() >= 15


def test_bwd_entry_points_reject_bad_arguments_before_launch():
    from tcs_mi355 import native
    L = native.lib()
    assert L.tcs_loss_finish_counts(None, 15, 1, 40, 40, 3, 3, None, None, None, None, None) == -1
    assert L.tcs_sequence_loss_bwd(None, 0, 0, 3, None, None, 0, None, None, 1, 40, 40, None, None, None, None, None, None, None) == -1
    assert L.tcs_init_loss_bwd(None, 10, None, None, 0, 1, 40, 40, 3, 0.5, None, None, None, None) == -1
    assert L.tcs_grad_normal_loss_bwd(None, 0, None, 0, 0, 3, None, None, None, None, None, None, 1, 40, 40, None, None, None, None, None,
                                      None) == -1


def test_train_losses_imports_without_core():
    code = ("import sys; import tcs_mi355.train_losses as t; assert not any(m == 'core' or m.startswith('core.') for m in sys.modules); "
            "assert all(hasattr(t, n) for n in ('sequence_loss', 'init_loss', 'disp_grad_loss', 'disp_normal_loss', "
            "'training_objective', 'loss_weights', 'gt_targets'))")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    subprocess.run([sys.executable, "-c", code], check=True, env=env)


def test_golden_inputs_are_make_loss_case():
    gold = golden()
    assert len(gold["cases"]) == 5
    for i, c in enumerate(gold["cases"]):
        assert H.digest(H.case_inputs(c)) == str(gold[f"c{i}_digest"]), i
    assert os.path.getsize(os.path.join(GOLDEN, "loss_grad.npz")) < 200 * 1024


@pytest.mark.parametrize("i", range(5))
def test_restatement_reproduces_the_reference_gradients(i):
    """Every gradient the reference's float32 autograd gives, to 1e-5 of the tensor's largest gradient, off the kinks (the reference
    needs none excluded on these cases; at most 0.1 % may be)."""
    gold = golden()
    c = [int(x) for x in gold["cases"][i]]
    grads, info = restate_grads(H.case_inputs(c), c[4], c[5], bool(c[6]))
    for part in ("total", "seq", "init", "norm", "grad"):
        for name, g64 in grads[part].items():
            key = f"c{i}_{part}_{name}"
            if key not in gold:
                assert part != "total" and i == 4, key
                continue
            ref = torch.from_numpy(gold[key]).double()
            assert ref.shape == g64.shape and bool(torch.isfinite(ref).all())
            keep = ~info["kinks"][name]
            assert int((~keep).sum()) <= 1e-3 * keep.numel(), (key, int((~keep).sum()))
            scale = float(g64.abs().max())
            err = float(((ref - g64).abs() * keep).max())
            print(f"{key}: max|g| {scale:.3e}  e_ref {err:.3e}  ({err / max(scale, 1e-300):.2e} of max)")
            assert err <= 1e-5 * scale, (key, err, scale)
            if c[7]:
                assert not ref.any() and not g64.any(), key


def test_empty_case_is_nan_loss_zero_gradient():
    gold = golden()
    i = [int(c[7]) for c in gold["cases"]].index(1)
    assert np.isnan(gold[f"c{i}_loss"]).all()
    assert all(not gold[f"c{i}_total_{n}"].any() for n in INPUTS)


def _cpu_case(iters=3):
    return H._cpu_case(iters)


def test_validation_matches_losses_and_grad_inputs_reach_the_device_check():
    from tcs_mi355 import losses, train_losses as tl
    c, out = _cpu_case()
    flow, valid = c["flow"], c["valid"]
    vmask = (valid >= 0.5).unsqueeze(1)
    w = tl.loss_weights(3)
    assert tl.loss_weights is losses.loss_weights and tl.gt_targets is losses.gt_targets          # re-exported, not copied
    g_out = dict(out, cost_volume=out["cost_volume"].clone().requires_grad_(True),
                 flow_mono=out["flow_mono"].clone().requires_grad_(True))
    # CPU tensors that require grad: accepted as differentiable inputs, then refused for being on the CPU
    with pytest.raises(RuntimeError, match="no CPU path"):
        tl.training_objective(g_out, flow, valid)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tl.init_loss(g_out["cost_volume"], flow, vmask, k=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tl.sequence_loss(g_out["flow_mono"], out["flow_init"], out["flow_predictions"], flow, vmask, w)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tl.disp_grad_loss([p.clone().requires_grad_(True) for p in out["disp_grad_q_predictions"]], torch.zeros(1, 2, 32, 48), vmask, w)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tl.disp_normal_loss([[p.clone().requires_grad_(True) for p in pair] for pair in out["flow_q_predictions"]],
                            torch.zeros(1, 3, 32, 48), vmask, w)
    # the ground truth and the mask get no gradient
    g = flow.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        tl.training_objective(out, g, valid)
    with pytest.raises(NotImplementedError):
        tl.sequence_loss(out["flow_mono"], out["flow_init"], out["flow_predictions"], g, vmask, w)
    with pytest.raises(NotImplementedError):
        tl.init_loss(out["cost_volume"], g, vmask, k=1)
    with pytest.raises(NotImplementedError):
        tl.disp_grad_loss(out["disp_grad_q_predictions"], torch.zeros(1, 2, 32, 48, requires_grad=True), vmask, w)
    with pytest.raises(NotImplementedError):
        tl.disp_normal_loss(out["flow_q_predictions"], torch.zeros(1, 3, 32, 48, requires_grad=True), vmask, w)
    # the forward's limits, raised before any launch
    with pytest.raises(ValueError, match="init_k"):
        tl.training_objective(g_out, flow, valid, init_k=13)
    with pytest.raises(ValueError, match="k="):
        tl.init_loss(g_out["cost_volume"], flow, vmask, k=9)
    with pytest.raises(ValueError, match="scale"):
        tl.disp_grad_loss(out["disp_grad_q_predictions"], torch.zeros(1, 2, 32, 48), vmask, w, scale=0.5)
    with pytest.raises(ValueError, match="lacks"):
        tl.training_objective({"flow_predictions": []}, flow, valid)
    with pytest.raises(ValueError, match="float32"):
        tl.init_loss(g_out["cost_volume"].double(), flow, vmask, k=1)


def test_stacking_keeps_the_gradient_path():
    """Views of a stacked leaf use the leaf itself; views made leaves of their own, and separate tensors, go through torch.stack."""
    from tcs_mi355 import losses
    base = torch.zeros(3, 2, 1, 1, 8, 8, requires_grad=True)
    pairs = [[base[i, 0], base[i, 1]] for i in range(3)]
    assert losses._stacked_pairs(pairs, (1, 1, 8, 8)) is base
    plain = torch.zeros(3, 2, 1, 1, 8, 8)
    assert losses._stacked_pairs([[plain[i, 0], plain[i, 1]] for i in range(3)], (1, 1, 8, 8)) is plain
    own = [[plain[i, 0].detach().requires_grad_(True), plain[i, 1]] for i in range(3)]
    s = losses._stacked_pairs(own, (1, 1, 8, 8))
    assert s is not plain and s.requires_grad and s.grad_fn is not None


def test_the_backward_path_never_reads_the_device_on_the_host():
    import inspect

    from tcs_mi355 import ops, train_losses
    src = inspect.getsource(train_losses._Objective.backward) + "".join(
        inspect.getsource(f) for f in (ops.sequence_loss_backward, ops.init_loss_backward, ops.grad_normal_loss_backward, ops._host_weights))
    for word in (".item(", ".cpu(", ".tolist(", "synchronize", ".numpy("):
        assert word not in src, word
