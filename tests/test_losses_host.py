"""The training objective on the host side (no GPU): the tcs_*loss* C ABI (symbols, ABI version, workspace query), the Python
surface's validation (it raises before any launch), loss_weights, and an fp64 restatement of train_stereo.py:41-180, 362-399 against
the reference's own numbers (tests/golden/losses.npz, tools/make_goldens_losses.py) on the seeded inputs of synth.make_loss_case.
test_gpu_losses.py holds the HIP path to the same restatement."""
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

NEW_SYMBOLS = ("tcs_loss_workspace_bytes", "tcs_loss_targets", "tcs_loss_targets_full", "tcs_sequence_loss", "tcs_init_loss",
               "tcs_grad_normal_loss", "tcs_loss_finish")
SEQ_KEYS = ("epe", "epe_refine", "epe_init", "1px", "3px", "5px", "1px_refine", "3px_refine", "5px_refine")
INIT_KEYS = ("init_loss", "init_gt_loss", "init_nm_loss", "forward_mask_rate")
RATE_KEYS = {"1px", "3px", "5px", "1px_refine", "3px_refine", "5px_refine", "forward_mask_rate"}


def golden():
    return dict(np.load(os.path.join(GOLDEN, "losses.npz")))


def case_inputs(c):
    from tcs_mi355 import synth
    seed, B, H, W, iters, k, dense, empty = (int(v) for v in c)
    return synth.make_loss_case(seed, B, H, W, iters, empty=bool(empty))


def digest(case):
    h = hashlib.sha256()
    for key in sorted(case):
        h.update(np.ascontiguousarray(case[key]).tobytes())
    return h.hexdigest()[:16]


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement: masks and targets with the reference's float32 ops (their rounding decides them), every loss value in float64
# ---------------------------------------------------------------------------------------------------------------------------------
def median_pool4(x):
    """MedianPool2d(4, 4) (core/utils/utils.py:121): the lower median of each 4x4 window."""
    u = x.unfold(2, 4, 4).unfold(3, 4, 4)
    return u.contiguous().view(u.size()[:4] + (-1,)).median(dim=-1)[0]


def grad_xy(d):
    """disp2disp_gradient_xy (geo_utils.py:115): replicate-padded forward differences, [B,2,H,W]."""
    p = F.pad(d, (1, 1, 1, 1), mode="replicate")
    return torch.cat((p[:, :, 1:-1, 2:] - p[:, :, 1:-1, 1:-1], p[:, :, 2:, 1:-1] - p[:, :, 1:-1, 1:-1]), 1)


def normal_xy(d):
    g = grad_xy(d)
    return F.normalize(torch.cat((g, -torch.ones_like(g[:, :1])), 1), dim=1)


def quarter_valid(v, dense):
    """The valid mask of disp_grad_loss / disp_normal_loss at quarter resolution (train_stereo.py:50-54)."""
    if dense:
        return F.max_pool2d(v.float(), 4, 4, 0).bool()
    return F.interpolate(v.float(), scale_factor=0.25, mode="bilinear", align_corners=True) == 1


def targets(flow, valid_raw):
    """(valid [B,1,H,W], grad GT pooled [B,2,h,w] + mask, normal GT pooled [B,3,h,w] + mask) as train_stereo.py:366-376, 46-48, 72-74."""
    mag = torch.sum(flow ** 2, dim=1).sqrt()
    v = ((valid_raw >= 0.5) & (mag < 700)).unsqueeze(1)
    g = median_pool4(grad_xy(-flow))
    n = median_pool4(normal_xy(-flow))
    gm = (g[:, :1] < 5) & (g[:, 1:] < 5)
    nm = (n[:, :1] / n[:, 2:] < 5) & (n[:, 1:2] / n[:, 2:] < 5)
    return v, g, gm, n, nm


def mean(x, m):
    return float(x[m].double().mean()) if bool(m.any()) else float("nan")


def restate(case, iters, k, dense, thres=0.5):
    """train_stereo.py:362-399 on one make_loss_case: {'seq', 'init', 'norm', 'grad', 'total'} laid out as losses.npz."""
    t = {key: torch.from_numpy(v) for key, v in case.items()}
    flow, up, q, gr = t["flow"], t["up"].double(), t["q"].double(), t["grad"].double()
    n = iters
    gam = 0.9 ** (15 / (n - 1))
    wts = [gam ** (n - i - 1) for i in range(n)]
    v, g, gm, nrm, nm = targets(flow, t["valid"])
    gt = flow.double()
    # sequence_loss
    seq = 0.1 * mean((t["flow_init"].double() - gt).abs(), v) + 0.1 * mean((t["flow_mono"].double() - gt).abs(), v)
    for i in range(n):
        seq += wts[i] * mean((up[i, 0] - gt).abs() + 1.2 * (up[i, 1] - gt).abs(), v)
    e = [((x - gt) ** 2).sum(1, keepdim=True).sqrt() for x in (up[-1, 0], up[-1, 1], t["flow_init"].double())]
    m = [mean(e[0], v), mean(e[1], v), mean(e[2], v)] + [mean((e[j] < th).double(), v) for j in (0, 1) for th in (1, 3, 5)]
    # init_loss
    cv = t["cost_volume"].double()
    B, D, h, w = cv.shape
    fs = 0.25 * F.interpolate(flow, scale_factor=0.25, mode="nearest")
    vi = (F.interpolate(v.float(), scale_factor=0.25, mode="bilinear", align_corners=True) == 1) & (fs.abs() < 175)
    idx = torch.arange(w).view(1, 1, 1, -1).double() + fs.double()
    mask = (idx >= 0) & (idx <= D - 1) & vi
    idx = idx.clamp(0, D - 1)
    df = idx.floor().long()
    fr = idx - df
    phi = fr * cv.gather(1, (df + 1).clamp(0, D - 1)) + (1 - fr) * cv.gather(1, df.clamp(0, D - 1))
    cand = torch.arange(D).view(1, -1, 1, 1).double()
    excl = ((cand >= idx - 1.5) & (cand < idx + 1.5)) | ~mask
    top = torch.topk(cv.masked_fill(excl, 0), k=k, dim=1).values
    gl = 1 - mean(phi, mask)
    nml = mean((top + thres - phi).clamp(min=0), mask.expand(-1, k, -1, -1))
    fmr = float(((top[:, :1] + 0.3 - phi) > 0).double().mean())
    # disp_grad_loss / disp_normal_loss
    qv = quarter_valid(v, dense)
    gv, nv = qv & gm, qv & nm
    grad = sum(wts[i] * mean((gr[i] - g.double()).abs().mean(1, keepdim=True), gv) for i in range(n))
    ng = nrm.double()

    def nl(f):
        p = normal_xy(-f)
        return 0.5 * (p - ng).abs().mean(1, keepdim=True) + 0.5 * (1 - (p * ng).sum(1, keepdim=True))
    norm = sum(wts[i] * (mean(nl(q[i, 0]), nv) + 1.2 * mean(nl(q[i, 1]), nv)) for i in range(n))
    return {"seq": [seq] + m, "init": [gl + nml, gl + nml, gl, nml, fmr], "norm": [norm, norm], "grad": [grad, grad],
            "total": [seq + gl + nml + 0.25 * norm + 5 * grad]}


def assert_matches(res, gold, i, rtol=1e-5):
    """Losses and EPEs to rtol; threshold rates and forward_mask_rate exactly (as float32); NaN where the golden is NaN."""
    for part, keys in (("seq", ("loss",) + SEQ_KEYS), ("init", ("loss",) + INIT_KEYS), ("norm", ("loss", "norm_loss")),
                       ("grad", ("loss", "grad_loss")), ("total", ("total",))):
        ref = gold[f"c{i}_{part}"]
        for j, key in enumerate(keys):
            a, b = float(res[part][j]), float(ref[j])
            if np.isnan(b):
                assert np.isnan(a), (i, part, key, a)
            elif key in RATE_KEYS:                      # the reference's rate is a float32 mean of exact counts
                assert np.float32(a) == np.float32(b), (i, part, key, a, b)
            else:
                assert abs(a - b) <= rtol * abs(b) + 1e-7, (i, part, key, a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_loss_symbols_declared_exported_and_abi_13():
    from tcs_mi355 import build, native
    build.build(verbose=False)
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "tcs_mi355.h")).read()
    L = native.lib()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header, name
        assert name in native.SIGNATURES, name
        assert hasattr(L, name), name
    assert L.tcs_abi_version() >= 13


def test_workspace_query_and_finish_rejects_bad_arguments():
    from tcs_mi355 import native
    L = native.lib()
    n = L.tcs_loss_workspace_bytes(1, 480, 640, 32)
    assert n > 0 and n % 8 == 0
    assert L.tcs_loss_workspace_bytes(1, 480, 640, 5) < n
    assert L.tcs_loss_workspace_bytes(1, 480, 640, 0) == 0
    assert L.tcs_loss_workspace_bytes(1, 480, 640, 65) == 0
    assert L.tcs_loss_workspace_bytes(1, 3, 640, 5) == 0
    # NULL pointers and bad k / modes are refused before anything is launched
    assert L.tcs_init_loss(None, 10, None, None, 0, 1, 40, 40, 3, 0.5, 1, None, None) == -1
    assert L.tcs_loss_finish(None, 15, 1, 40, 40, 3, 3, None, None, None, None) == -1
    assert L.tcs_loss_targets(None, None, 3, 1, 40, 40, None, None, None, None, None, None, None) == -1


def test_loss_weights():
    from tcs_mi355.losses import loss_weights
    for n in (2, 5, 32):
        g = 0.9 ** (15 / (n - 1))
        assert loss_weights(n) == [g ** (n - i - 1) for i in range(n)]
    w = loss_weights(5)
    assert w[-1] == 1.0 and all(a < b for a, b in zip(w, w[1:]))
    for n in (0, 1):
        with pytest.raises((ValueError, ZeroDivisionError)):
            loss_weights(n)


def _cpu_case(iters=3, B=1, H=32, W=48):
    from tcs_mi355 import synth
    c = {key: torch.from_numpy(v) for key, v in synth.make_loss_case(5, B, H, W, iters).items()}
    out = {"flow_predictions": [[c["up"][i, 0], c["up"][i, 1]] for i in range(iters)],
           "flow_q_predictions": [[c["q"][i, 0], c["q"][i, 1]] for i in range(iters)],
           "disp_grad_q_predictions": [c["grad"][i] for i in range(iters)],
           "flow_mono": c["flow_mono"], "flow_init": c["flow_init"], "cost_volume": c["cost_volume"]}
    return c, out


def test_validation_before_launch():
    """Every entry point raises on CPU tensors, bad shapes, k > min(8, D), unsupported scales and grad inputs, with no GPU."""
    from tcs_mi355 import losses
    c, out = _cpu_case()
    flow, valid = c["flow"], c["valid"]
    vmask = (valid >= 0.5).unsqueeze(1)
    w = losses.loss_weights(3)
    with pytest.raises(RuntimeError, match="HIP device"):
        losses.training_objective(out, flow, valid)
    with pytest.raises(RuntimeError, match="HIP device"):
        losses.sequence_loss(out["flow_mono"], out["flow_init"], out["flow_predictions"], flow, vmask, w)
    with pytest.raises(ValueError, match="k="):
        losses.init_loss(out["cost_volume"], flow, vmask, k=9)
    with pytest.raises(ValueError, match="k="):
        losses.init_loss(out["cost_volume"][:, :2], flow, vmask, k=3)
    with pytest.raises(ValueError, match="init_k"):
        losses.training_objective(out, flow, valid, init_k=13)
    with pytest.raises(ValueError, match="scale"):
        losses.disp_grad_loss(out["disp_grad_q_predictions"], torch.zeros(1, 2, 32, 48), vmask, w, scale=0.5)
    with pytest.raises(ValueError, match="n_downsample"):
        losses.training_objective(out, flow, valid, n_downsample=3)
    with pytest.raises(ValueError):
        losses.sequence_loss(out["flow_mono"], out["flow_init"], out["flow_predictions"], flow, vmask[:, :, :16], w)
    with pytest.raises(ValueError, match="cost_volume"):
        losses.init_loss(out["cost_volume"][:, :, :4], flow, vmask, k=1)
    with pytest.raises(ValueError, match="lacks"):
        losses.training_objective({"flow_predictions": []}, flow, valid)
    with pytest.raises(ValueError):
        losses.disp_normal_loss(out["flow_q_predictions"], torch.zeros(1, 3, 32, 40), vmask, w)
    g = flow.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        losses.training_objective(out, g, valid)
    with pytest.raises(NotImplementedError):
        losses.sequence_loss(out["flow_mono"], out["flow_init"], out["flow_predictions"], g, vmask, w)
    cvg = out["cost_volume"].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        losses.init_loss(cvg, flow, vmask, k=1)
    with pytest.raises(NotImplementedError):
        losses.disp_grad_loss([p.clone().requires_grad_(True) for p in out["disp_grad_q_predictions"]], torch.zeros(1, 2, 32, 48),
                              vmask, w)


def test_make_loss_case_reproduces_the_golden_inputs():
    gold = golden()
    for i, c in enumerate(gold["cases"]):
        assert digest(case_inputs(c)) == str(gold[f"c{i}_digest"]), i


def test_golden_covers_the_cases_the_issue_names():
    cases = golden()["cases"]
    assert {int(c[6]) for c in cases} == {0, 1}          # dense_gt both ways
    assert {int(c[5]) for c in cases} >= {1, 3}          # k
    assert {int(c[1]) for c in cases} == {1, 2}          # B
    assert any(int(c[7]) for c in cases)                 # an empty mask
    assert os.path.getsize(os.path.join(GOLDEN, "losses.npz")) < 150 * 1024


@pytest.mark.parametrize("i", range(4))
def test_restatement_matches_the_reference(i):
    gold = golden()
    c = gold["cases"][i]
    res = restate(case_inputs(c), int(c[4]), int(c[5]), bool(c[6]))
    assert_matches(res, gold, i)


def test_gt_targets_matches_the_trainer():
    from tcs_mi355.losses import gt_targets
    c, _ = _cpu_case()
    v, g, n = gt_targets(c["flow"], c["valid"])
    mag = torch.sum(c["flow"] ** 2, dim=1).sqrt()
    assert torch.equal(v, ((c["valid"] >= 0.5) & (mag < 700)).unsqueeze(1))
    assert torch.equal(g, grad_xy(-c["flow"]))
    assert torch.equal(n, normal_xy(-c["flow"]))
